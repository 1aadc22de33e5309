"""ARCVAETrainerWithLoss on MI355X (reference trainer.py:12-736).

Same constructor, schedules, epoch structure, `history` keys, checkpoint file names and the same
consumption order of NumPy's global RNG stream (batch shuffles and teacher-forcing coins, SURVEY
Q5/Q16), so an epoch visits the same batches with the same coins as the reference would.  The
step itself (loss, gradients, two un-bias-corrected Adam updates; trainer.py:292-333) is one
captured hipGraph replay of the arcvae_hip engine.

Reproduced on purpose: by default gradient clipping is a no-op (Q6: the reference's `_clip_gradients` sums
nothing, so `grad_clip` never changes a gradient); a "loss explosion" only drops the value from
the running mean, the update has already been applied (Q15); every 25th batch a second forward is
run for logging with post-update weights and T more coins (Q16).

Global-norm clipping (an extension): `grad_clip_mode="global_norm"` applies the reference's
intended rule with max_norm = `grad_clip` (<= 0: no clipping, as the reference's `if self.grad_clip > 0`) inside the
captured step -- norm over every gradient of the step, predictor included, scale = max_norm / (norm + 1e-8) when the norm
exceeds max_norm.  `history["grad_norm"]` then holds the epoch mean of the pre-clip norms, read with the per-batch loss
(no extra host sync).  `grad_clip_mode="reference"` (default) keeps the no-op and the history keys as they are.
Checkpoints: same file names, but a flat non-pickle .npz keyed by the parameter names (Q21).

Property predictor (an extension; the reference's own branch cannot run, Q10): with
`property_predictor=` a models.PropertyPredictor, the step also trains it (its own Adam, same lr, no bias correction),
lambda_prop weighs its loss, train_prop / val_prop are real, and the checkpoints carry `predictor_weights/<name>` and
`predictor_optimizer_state/{m,v}/<name>`.  Not combined with data parallelism (refused).

Learning-rate schedules (an extension): with `lr_schedule=` an lr_schedule.LRSchedule the rate of
every step is schedule.lr(global_step) -- global_step counts every step the trainer launched -- handed to the step as a device
word (lr_device=True: the same captured step replays at every rate).  history["learning_rate"] then holds the rate of each
epoch's last step, and the checkpoints carry `global_step` and `lr_schedule_json`, so a resumed run continues the curve.
`lr_schedule=None` (default) is the one-rate trainer, launch for launch, with the checkpoint keys as they are.

Weight EMA (an extension): with `ema_decay=` a decay in (0, 1) the trainer keeps an exponential moving
average of every module's weights on the device (arcvae_hip.ema.WeightEMA): one launch right behind every step, outside the
captured step, skipped on the device together with an Adam update that was skipped.  `ema_warmup=True` ramps the decay as
min(decay, (1 + t) / (10 + t)); `ema_eval=True` runs the epoch's evaluations (true train loss, validation, latent stats) on the
averaged weights, so the history and train.py's choice of checkpoint_best follow them.  Checkpoints then also carry
`{tag}_ema_weights/<name>` and `ema_json`; the raw weights stay under their keys, so a resume continues training.
`ema_decay=None` (default): no EMA object, no launch, no key.

Data parallelism (the reference is single-process): under `torch.distributed` (train.py started by
`python -m torch.distributed.run`, one process per GPU) every rank runs THIS epoch flow on the same dataset order and the
same coins (one seeded NumPy stream), every batch is the GLOBAL batch, and the step / the loss forwards work on the
rank's row shard with the stats seam and the gradient buckets all-reduced over RCCL (arcvae_hip.dp.EngineDataParallel,
enabled by `api.enable_data_parallel`).  The loss scalars every rank logs are the global batch's, so the history is the
single-process history; rank 0 alone prints and writes checkpoints / history / plots.
"""
from __future__ import annotations

import contextlib
import json
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from arcvae_hip import api
from complete_vae_loss import complete_vae_loss

try:  # progress bars are cosmetic
    from tqdm import tqdm
except Exception:  # pragma: no cover
    def tqdm(it, **kw):
        return it


class ARCVAETrainerWithLoss:
    def __init__(self, encoder, decoder, property_predictor, dataset, learning_rate: float = 1e-4,
                 batch_size: int = 32, beta_start: float = 0.0, beta_end: float = 0.4,
                 beta_warmup_epochs: int = 100, lambda_prop: float = 0.1, lambda_collapse: float = 0.01,
                 free_bits: float = 0.5, lambda_mi: float = 0.01, grad_clip: float = 1.0,
                 checkpoint_dir: str = "./checkpoints", progress: bool = True, grad_clip_mode: str = "reference",
                 lr_schedule=None, ema_decay: Optional[float] = None, ema_warmup: bool = False, ema_eval: bool = False):
        self.encoder, self.decoder, self.property_predictor = encoder, decoder, property_predictor
        self.dataset, self.batch_size, self.grad_clip = dataset, batch_size, grad_clip
        if grad_clip_mode not in ("reference", "global_norm"):
            raise ValueError(f"grad_clip_mode must be 'reference' or 'global_norm', got {grad_clip_mode!r}")
        self.grad_clip_mode = grad_clip_mode
        # max_norm of the step's global-norm clip, or None: the reference's no-op (Q6)
        self.clip_norm = float(grad_clip) if (grad_clip_mode == "global_norm" and grad_clip > 0) else None
        self.lambda_prop, self.lambda_collapse = lambda_prop, lambda_collapse
        self.free_bits, self.lambda_mi = free_bits, lambda_mi
        self.beta_start, self.beta_end, self.beta_warmup_epochs = beta_start, beta_end, beta_warmup_epochs
        self.learning_rate = learning_rate
        if lr_schedule is not None:
            from lr_schedule import LRSchedule
            if not isinstance(lr_schedule, LRSchedule):
                raise ValueError(f"lr_schedule must be an lr_schedule.LRSchedule or None, got {type(lr_schedule).__name__}")
        self.lr_schedule = lr_schedule
        self.global_step = 0         # steps launched so far (schedule mode; batches the explosion check skips included)
        self.last_lr = None          # the rate of the last step launched (schedule mode)
        self.checkpoint_dir = Path(checkpoint_dir)
        self.checkpoint_dir.mkdir(exist_ok=True)
        self.progress = progress
        self.persist_best_val = False  # Q21: the reference never writes best_val_loss
        self.best_val_loss = float("inf")
        self.engine = self._make_engine(encoder, decoder)
        self.rank, self.world = self._rank_world()
        if self.rank != 0:
            self.progress = False
        # set when a step reported a lost stream order: the encoder's update was skipped on the device, but the decoder's
        # (applied ~1 ms earlier, at the end of its own segment) may already be in -- the two modules can be one step
        # apart, so this state is never checkpointed
        self.poisoned = False
        self.history = {k: [] for k in (
            "epoch", "train_loss", "train_recon", "train_kl", "train_collapse", "train_prop", "val_loss",
            "val_recon", "val_kl", "val_collapse", "val_prop", "beta", "teacher_forcing", "learning_rate",
            "mutual_info")}
        if self.clip_norm is not None:
            self.history["grad_norm"] = []
        # weight EMA (arcvae_hip/ema.py): None = the trainer as it was, launch for launch
        if ema_decay is None and (ema_warmup or ema_eval):
            raise ValueError("ema_warmup / ema_eval need ema_decay")
        self.ema, self.ema_eval = None, bool(ema_eval)
        if ema_decay is not None:
            from arcvae_hip.ema import WeightEMA, check_decay
            check_decay(ema_decay)
            self.ema = WeightEMA({tag: mod.store for tag, mod in self._modules()}, ema_decay, warmup=ema_warmup)
            if self.engine is not None:
                api.attach_ema(self.encoder, self.decoder, self.ema)

    # ---- the three calls into the step engine (tests drive the same epoch flow with oracle-backed ones) ----------
    def _make_engine(self, encoder, decoder):
        return api.engine_for(encoder, decoder, self.property_predictor)

    def _rank_world(self) -> Tuple[int, int]:
        dp = api.data_parallel_of(self.encoder, self.decoder)
        return (dp.rank, dp.world) if dp is not None else (0, 1)

    def _train_step(self, molecules, conditions, teacher_forcing_ratio: float, hyper: Dict[str, float]):
        """loss + grads + (no-op clip, Q6, or the global-norm clip) + both Adam updates: one captured step (N ranks:
        arcvae_hip.dp).  Returns [total_loss, step status] of the GLOBAL batch as one tensor -- [total_loss, step status,
        pre-clip norm] with the global-norm clip: read together, one host sync per batch."""
        rate = {}
        if self.lr_schedule is not None:     # the schedule's rate of this step, as a device word
            self.last_lr = self.lr_schedule.lr(self.global_step)
            self.global_step += 1
            rate = dict(lr_device=True)
        out, _ = api.value_and_grad(self.encoder, self.decoder, molecules, conditions,
                                    teacher_forcing_ratio=teacher_forcing_ratio,
                                    lr=self.last_lr if self.lr_schedule is not None else self.learning_rate,
                                    predictor=self.property_predictor, grad_clip=self.clip_norm, **rate, **hyper)
        if self.ema is not None:
            # one plain launch on the step's stream, behind every Adam update of the step (api.last_step_guards says why) and
            # ahead of the per-batch .tolist(): the host never waits for it
            self.ema.update(guards=api.last_step_guards(self.encoder, self.decoder, self.property_predictor))
        return out["loss_status_norm"] if self.clip_norm is not None else out["loss_and_status"]

    def _encode(self, molecules, conditions):
        return self.encoder(molecules, conditions)

    # ---- schedules (trainer.py:102-114) ------------------------------------------------------
    def compute_beta(self, epoch: int) -> float:
        if epoch < self.beta_warmup_epochs:
            return float(self.beta_start + (self.beta_end - self.beta_start) * (epoch / self.beta_warmup_epochs))
        return float(self.beta_end)

    def compute_teacher_forcing_ratio(self, epoch: int, total_epochs: int) -> float:
        return float(max(0.5, 0.9 - 0.4 * (epoch / total_epochs)))

    # ---- helpers -------------------------------------------------------------------------------
    def _hyper(self, beta: float) -> Dict[str, float]:
        h = dict(beta=beta, lambda_collapse=self.lambda_collapse, lambda_mi=self.lambda_mi, target_mi=4.85,
                 free_bits=self.free_bits)
        if self.property_predictor is not None:
            h["lambda_prop"] = self.lambda_prop
        return h

    def _loss_dict(self, molecules, conditions, beta: float, tf: float) -> Dict[str, torch.Tensor]:
        return complete_vae_loss(self.encoder, self.decoder, self.property_predictor, molecules, conditions, beta=beta,
                                 lambda_prop=self.lambda_prop, lambda_collapse=self.lambda_collapse,
                                 teacher_forcing_ratio=tf, free_bits=self.free_bits, lambda_mi=self.lambda_mi,
                                 target_mi=4.85)

    def _eval_batches(self, dataset, beta: float, limit: Optional[int], desc: str) -> Dict[str, float]:
        tot = dict(loss=0.0, recon=0.0, kl=0.0, collapse=0.0, prop=0.0)
        n = 0
        it = dataset.to_batches(self.batch_size, shuffle=False)
        if self.progress and limit is None:
            it = tqdm(it, total=len(dataset) // self.batch_size, desc=desc)
        for bi, (mol, cond) in enumerate(it):
            if limit is not None and bi >= limit:
                break
            d = self._loss_dict(mol, cond, beta, 0.0)  # teacher_forcing_ratio = 0.0: pure argmax chain
            vals = torch.stack([d["total_loss"], d["recon_loss"], d["kl_loss"], d["collapse_penalty"],
                                d["prop_loss"]]).tolist()  # one host sync per batch
            for k, v in zip(("loss", "recon", "kl", "collapse", "prop"), vals):
                tot[k] += v
            n += 1
        return {k: (v / n if n > 0 else 0.0) for k, v in tot.items()}

    def _eval_weights(self):
        """The weights the epoch's evaluations read: the averaged ones inside this context with ema_eval, else the raw ones."""
        return self.ema.applied() if (self.ema is not None and self.ema_eval) else contextlib.nullcontext()

    def _compute_true_train_loss(self, epoch: int, num_batches: int = 10) -> Dict[str, float]:
        """trainer.py:116-175: training loss WITHOUT teacher forcing on the first `num_batches` batches."""
        with self._eval_weights():
            return self._eval_batches(self.dataset, self.compute_beta(epoch), num_batches, "True train loss")

    def _validate(self, val_dataset, beta: float) -> Dict[str, float]:
        """trainer.py:418-487."""
        with self._eval_weights():
            return self._eval_batches(val_dataset, beta, None, "Validating")

    # ---- epoch -------------------------------------------------------------------------------------
    def train_epoch(self, epoch: int, total_epochs: int, val_dataset=None) -> Dict[str, float]:
        beta = self.compute_beta(epoch)
        tf = self.compute_teacher_forcing_ratio(epoch, total_epochs)
        if self.lr_schedule is not None and self.lr_schedule.total_steps is None:
            self.lr_schedule.set_total_steps(total_epochs * (len(self.dataset) // self.batch_size))
        self.last_train_metrics = self._train_epoch_batches(beta, tf)
        if self.lr_schedule is not None:
            self.history["learning_rate"].append(self.last_lr)       # the rate of the epoch's last step
        extra = {"grad_norm": self.last_train_metrics["grad_norm"]} if "grad_norm" in self.last_train_metrics else {}
        if self.engine is not None:
            self.engine.check_gates()  # a device-side gate that expired would mean the step's streams lost their order
        true_train = self._compute_true_train_loss(epoch, num_batches=20)
        val = self._validate(val_dataset, beta) if val_dataset is not None else dict(
            loss=0.0, recon=0.0, kl=0.0, collapse=0.0, prop=0.0)
        mu, logvar = self._get_latent_stats()
        mi_value = float(self._compute_mutual_information(mu, logvar))
        return {
            "train_loss": true_train["loss"], "train_recon": true_train["recon"], "train_kl": true_train["kl"],
            "train_collapse": true_train["collapse"], "train_prop": true_train["prop"],
            "val_loss": val.get("loss", 0.0), "val_recon": val.get("recon", 0.0), "val_kl": val.get("kl", 0.0),
            "val_collapse": val.get("collapse", 0.0), "val_prop": val.get("prop", 0.0), "beta": beta,
            "teacher_forcing": tf, "mutual_info": mi_value, **extra,
        }

    def _train_epoch_batches(self, beta: float, teacher_forcing_ratio: float) -> Dict[str, float]:
        """trainer.py:242-416."""
        total_loss, num_batches = 0.0, 0
        sums = dict(recon=0.0, kl=0.0, collapse=0.0, prop=0.0)
        comp_count = 0
        norms = []               # pre-clip norms of the epoch's steps (global-norm clip only)
        hyper = self._hyper(beta)
        it = self.dataset.to_batches(self.batch_size, shuffle=True)
        if self.progress:
            it = tqdm(it, total=len(self.dataset) // self.batch_size, desc="Training batches")
        for batch_idx, (molecules, conditions) in enumerate(it):
            loss_st = self._train_step(molecules, conditions, teacher_forcing_ratio, hyper)
            nst = int(loss_st.numel())   # 2, or 3 with the global-norm clip's norm
            if batch_idx == 0 or batch_idx % 25 == 0:  # Q16: second forward, post-update weights, T more coins
                d = self._loss_dict(molecules, conditions, beta, teacher_forcing_ratio)
                vals = torch.cat([loss_st, torch.stack([d["recon_loss"], d["kl_loss"], d["collapse_penalty"],
                                                        d["prop_loss"]])]).tolist()
                loss_val, status = vals[0], vals[1]
                for k, v in zip(("recon", "kl", "collapse", "prop"), vals[nst:]):
                    sums[k] += v
                comp_count += 1
            else:
                vals = loss_st.tolist()  # the reference syncs here too (trainer.py:366)
                loss_val, status = vals[0], vals[1]
            if nst == 3:
                norms.append(vals[2])
            if status != 0.0:
                # a device-side gate expired or a persistent sweep gave up in THIS step: the device has already
                # skipped both Adam updates (the weights are those of the previous batch); stop here, not at epoch end
                self.poisoned = True
                if self.engine is not None:
                    self.engine.check_gates()
                raise RuntimeError(f"training step {batch_idx}: stream order was lost on the device (the encoder's update "
                                   "was skipped; the decoder's may already be applied: do not checkpoint this state)")
            if not np.isfinite(loss_val) or loss_val > 2000.0 or loss_val < -10.0:  # Q15
                if self.rank == 0:
                    print(f"\nWARNING: loss explosion detected at batch {batch_idx}: {loss_val:.2e} "
                          "(update already applied; value excluded from the epoch mean)")
                self._loss_dict(molecules, conditions, beta, teacher_forcing_ratio)  # reference re-evaluates here
                continue
            total_loss += loss_val
            num_batches += 1
        out = {"loss": total_loss / max(1, num_batches),
               **{k: (v / comp_count if comp_count > 0 else 0.0) for k, v in sums.items()}}
        if self.clip_norm is not None:
            out["grad_norm"] = float(np.mean(norms)) if norms else 0.0
        return out

    @staticmethod
    def _clip_gradients(grads, max_norm: float = 1.0) -> Tuple:
        """trainer.py:490-522 sums only top-level arrays of the two grad trees; every top-level entry is a
        sub-module dict, so the norm is 0 and the gradients are returned unchanged (Q6) -- the default
        (grad_clip_mode="reference").  The rule it meant to apply is the opt-in grad_clip_mode="global_norm", which runs
        inside the captured step (api.value_and_grad(grad_clip=), csrc/clip.hip), not here."""
        return grads

    def _get_latent_stats(self):
        """trainer.py:524-545: encoder pass on the first 64 training rows, printed summary."""
        molecules, conditions = next(iter(self.dataset.to_batches(64, shuffle=False)))
        with self._eval_weights():
            mu, logvar = self._encode(molecules, conditions)      # (N ranks: every rank encodes the same 64 rows)
        if self.rank == 0:
            m, lv = mu.cpu().numpy(), logvar.cpu().numpy()
            print(f"   Latent Stats: mu=[{m.min():.3f}, {m.max():.3f}] (mean={m.mean():.3f}, std={m.std():.3f}), "
                  f"logvar=[{lv.min():.3f}, {lv.max():.3f}] (mean={lv.mean():.3f}, std={lv.std():.3f})")
        return mu, logvar

    @staticmethod
    def _compute_mutual_information(mu, logvar) -> float:
        """trainer.py:547-575: the monitoring variant with log(mean_var + 1e-8) (Q20).  The batch sums come
        from the device (arcvae_latent_stats); the 2Z+3 numbers are finished on the host."""
        from losses._dev import latent_stats
        stats, _, B, Z = latent_stats(mu, logvar, 0.0)
        s = stats.cpu().numpy().astype(np.float32)
        f = np.float32
        mean_mu, mean_var = s[:Z] / f(B), s[Z:2 * Z] / f(B)
        agg = f(-0.5) * np.sum(f(1.0) + np.log(mean_var + f(1e-8)) - mean_mu * mean_mu - mean_var, dtype=np.float32)
        return float(max(s[2 * Z] / f(B) - agg, f(0.0)))

    # ---- checkpoints / history (trainer.py:577-736) -----------------------------------------------------
    def _modules(self):
        mods = [("encoder", self.encoder), ("decoder", self.decoder)]
        if self.property_predictor is not None:
            mods.append(("predictor", self.property_predictor))
        return mods

    def save_checkpoint(self, epoch: int, is_best: bool = False):
        if self.poisoned:
            raise RuntimeError("a training step lost its stream order (encoder and decoder may be one update apart): "
                               "refusing to checkpoint this state; resume from the last checkpoint")
        if self.rank != 0:       # N ranks hold identical weights and optimizer state: rank 0 writes
            return
        ck = {"epoch": np.array(epoch), "history_json": np.array(json.dumps(self.history))}
        for tag, mod in self._modules():
            st = mod.store
            for n in st.names():
                ck[f"{tag}_weights/{n}"] = st.p(n).cpu().numpy()
                ck[f"{tag}_optimizer_state/m/{n}"] = st._view(st.adam_m, n).cpu().numpy()
                ck[f"{tag}_optimizer_state/v/{n}"] = st._view(st.adam_v, n).cpu().numpy()
        if self.ema is not None:     # the averaged weights beside the raw ones (which stay under their keys: a resume trains on)
            for tag, mod in self._modules():
                for n in mod.store.names():
                    ck[f"{tag}_ema_weights/{n}"] = self.ema.shadow_view(tag, n).cpu().numpy()
            ck["ema_json"] = np.array(json.dumps(self.ema.state()))
        ck["learning_rate"] = np.array(self.learning_rate)
        if self.lr_schedule is not None:
            ck["global_step"] = np.array(self.global_step)
            ck["lr_schedule_json"] = np.array(json.dumps(self.lr_schedule.state()))
        if self.persist_best_val:
            ck["best_val_loss"] = np.array(self.best_val_loss)
        if is_best:
            self._save_checkpoint(ck, self.checkpoint_dir / "checkpoint_best.npz")
        self._save_checkpoint(ck, self.checkpoint_dir / f"checkpoint_epoch_{epoch:03d}.npz")

    @staticmethod
    def _save_checkpoint(checkpoint: dict, path: Path):
        np.savez(str(path), **checkpoint)
        print(f"    Saved checkpoint: {path}")

    def load_checkpoint(self, checkpoint_path: str) -> int:
        ck = np.load(checkpoint_path, allow_pickle=False)
        for tag, mod in self._modules():     # (a checkpoint without predictor_* keys leaves the predictor as it is)
            st = mod.store
            for n in st.names():
                if f"{tag}_weights/{n}" in ck:
                    st.p(n).copy_(torch.from_numpy(ck[f"{tag}_weights/{n}"]))
                if f"{tag}_optimizer_state/m/{n}" in ck:
                    st._view(st.adam_m, n).copy_(torch.from_numpy(ck[f"{tag}_optimizer_state/m/{n}"]))
                    st._view(st.adam_v, n).copy_(torch.from_numpy(ck[f"{tag}_optimizer_state/v/{n}"]))
        if "history_json" in ck:
            self.history = json.loads(str(ck["history_json"]))
        if self.lr_schedule is not None and "global_step" in ck:     # continue the curve where the run stopped
            from lr_schedule import LRSchedule
            self.global_step = int(ck["global_step"])
            self.lr_schedule = LRSchedule.from_state(json.loads(str(ck["lr_schedule_json"])))
        if self.ema is not None:     # (without an EMA the extra keys of an EMA checkpoint are ignored)
            if "ema_json" in ck:
                for tag, mod in self._modules():
                    for n in mod.store.names():
                        if f"{tag}_ema_weights/{n}" in ck:
                            self.ema.shadow_view(tag, n).copy_(torch.from_numpy(ck[f"{tag}_ema_weights/{n}"]))
                self.ema.load_state(json.loads(str(ck["ema_json"])))
            else:
                self.ema.reset()
                if self.rank == 0:
                    print("    checkpoint holds no weight EMA: the average restarts from the loaded weights (num_updates = 0)")
        return int(ck["epoch"]) if "epoch" in ck else 0

    def save_history(self, path: str):
        if self.rank != 0:
            return
        p = Path(path) / "training_history.json"
        with open(p, "w") as f:
            json.dump(self.history, f, indent=2)
        print(f"    Saved history: {p}")

    def plot_history(self, save_path: str = None):
        if self.rank != 0:
            return
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            print("    matplotlib not available for plotting")
            return
        h = self.history
        panels = [("Total Loss", [("train_loss", "Train"), ("val_loss", "Val")]),
                  ("Loss Components", [("train_recon", "Recon"), ("train_kl", "KL")]),
                  ("Posterior Collapse Penalty", [("train_collapse", "Collapse Penalty")]),
                  ("Property Prediction Loss", [("train_prop", "Train"), ("val_prop", "Val")]),
                  ("Annealing Schedules", [("beta", "Beta"), ("teacher_forcing", "TF Ratio")]),
                  ("Latent Space Health", [("mutual_info", "MI")])]
        fig, axes = plt.subplots(2, 3, figsize=(15, 10))
        for ax, (title, series) in zip(axes.ravel(), panels):
            for key, label in series:
                ax.plot(h["epoch"], h[key], label=label)
            if title == "Latent Space Health":
                ax.axhline(y=4.85, color="r", linestyle="--", label="Target")
                ax.axhline(y=1.0, color="orange", linestyle="--", label="Collapse")
            ax.set_xlabel("Epoch")
            ax.set_title(title)
            ax.legend()
            ax.grid(True, alpha=0.3)
        plt.tight_layout()
        if save_path:
            plt.savefig(save_path, dpi=150)
            print(f"    Saved plot: {save_path}")
        plt.close(fig)
