"""MLXAutoregressiveDecoderSampling on MI355X (reference models/decoder_sampling.py:6-129).

Owns its OWN, never-trained decoder (Q9: not weight-shared with ARCVAE.decoder); "temperature
sampling" is argmax(softmax(logits / T)) = greedy; tokens after EOS are still generated; with
early stopping the output is cut where every row has emitted EOS.  One dense decoder pass
(B*V rows) + one table walk replaces the reference's max_length dependent steps and its per-step
host sync; `load_from_decoder` is an explicit extension to sample from trained weights, and `sample=True` the true categorical
sampling the reference marks TODO (decoder_sampling.py:115-116): an extension with no reference behaviour to match.  So is
`generate_beam` (beam search with scores, csrc/beam.hip); `decoder.sequence_log_prob` scores given sequences; and
`sample=True` with `top_k` / `top_p` (truncated sampling, csrc/sample.hip) and with `min_p` / `typical_p` / `min_length`
(min-p, locally typical and minimum-length sampling, same file); and `generate_map` / `token_marginals` /
`length_distribution`: the exact most probable sequence and the exact per-step token and length distributions of the chain the
dense table defines (csrc/chain.hip); and `generate_kbest`: the exact K most probable sequences of that chain (csrc/kbest.hip);
and `length_penalty=` on both (the exact optimum of the length-normalised score), `best_by_length` (the best score of every
length) and `generate_of_length` (the most probable sequence of a given length); and `generate_without_replacement`: K distinct
random sequences per row, exactly a sample without replacement, with `importance_weights` for unbiased estimates (csrc/swor.hip);
and `sequence_entropy` / `sequence_divergence` / `expected_token_counts` / `expected_length`: the exact entropy, cross-entropy
and KL of the distribution over whole sequences and its expected token counts and length, closed forms on the forward recursion
(csrc/table.hip row costs, csrc/chain.hip expectations; `_expect` is their one path); and `generate_many`: N independent draws
per condition row from one dense table, the i.i.d. sampler of the list walk's measure (csrc/sample.hip, one thread per draw).

Every method is its argument checks, the decoder's one path to the table -- `load_conditions`, `dense_table`, `table_lse`,
`scratch` (models/decoder.py) -- and its own kernel.  What the methods share beyond that is written once below: `_state` +
`_launch` (the per-key buffers in `self._graphs` and the eager / capture / replay protocol of the two captured walks),
`_check_lengths`, `_check_chain`, `_length_divisors`, `_table`, `_outputs`, `_profile`, and `_cut` / `_stopped` (early
stopping).  A further decoder of the table is one method of that shape."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from arcvae_hip._lib import call, ptr, stream_ptr

from .decoder import MLXAutoregressiveDecoder, check_temperature


class MLXAutoregressiveDecoderSampling:
    def __init__(self, vocab_size: int, embedding_dim: int = 256, hidden_dim: int = 512, latent_dim: int = 200,
                 num_conditions: int = 6, num_layers: int = 3, pad_token: int = 0, end_token: int = 2, device=None,
                 generator=None):
        self.decoder = MLXAutoregressiveDecoder(vocab_size, embedding_dim, hidden_dim, latent_dim, num_conditions,
                                                num_layers, pad_token, end_token, device=device, generator=generator)
        self.vocab_size, self.embedding_dim, self.hidden_dim = vocab_size, embedding_dim, hidden_dim
        self.latent_dim, self.num_conditions = latent_dim, num_conditions
        self.pad_token, self.end_token = pad_token, end_token
        self._graphs = {}
        self._divisors = {}

    def load_from_decoder(self, other: MLXAutoregressiveDecoder, ema=None) -> None:
        """Extension (absent in the reference): copy trained decoder weights into the sampler.  ema (an
        arcvae_hip.ema.WeightEMA that tracks `other` as "decoder"): copy the decoder's averaged weights instead."""
        if ema is None:
            self.decoder.store.flat.copy_(other.store.flat)
            return
        if ema.stores.get("decoder") is not other.store:
            raise ValueError("load_from_decoder(ema=): the WeightEMA does not track this decoder's store as 'decoder'")
        self.decoder.store.flat.copy_(ema.shadow("decoder"))

    def parameters(self):
        return {"decoder": self.decoder.parameters()}

    def generate_with_temperature(self, z, conditions, max_length: int = 80, temperature: float = 1.0,
                                  early_stopping: bool = True, use_graph: bool = True, *, sample: bool = False,
                                  seed: int = 0, top_k=None, top_p=None, min_p=None, typical_p=None,
                                  min_length: int = 0) -> torch.Tensor:
        """[B, t_stop] int32 tokens (models/decoder_sampling.py:48-128).  z is accepted and unused (Q2).
        sample=True (keyword-only extension; the default reproduces the reference's greedy "temperature sampling", Q9): every token is
        DRAWN from softmax(logits / temperature) -- what decoder_sampling.py:115-116 leaves as a TODO -- with a counter-based
        generator keyed by (seed, row, step): the same seed returns the same molecules.
        top_k / top_p (keyword-only extension, with sample=True): draw from the truncated distribution instead -- the top_k most
        likely tokens (ties to the lower token), then the smallest prefix of them holding top_p of their renormalised mass
        (include/arcvae_hip.h arcvae_dec_sample_chain_topkp).  None = no truncation of that kind; both None = the categorical path.
        min_p / typical_p / min_length (keyword-only extension, with sample=True; include/arcvae_hip.h
        arcvae_dec_sample_chain_trunc): min_p keeps the tokens whose probability is at least min_p times the row's largest (on top
        of top_k / top_p; 0.0 = off); typical_p keeps the smallest prefix, holding typical_p of the top_k tokens' mass, of the
        tokens ordered by |log p + H|, H the row's entropy (locally typical sampling; 1.0 = off; not together with top_p or
        min_p); min_length > 0 masks the end token at the steps t < min_length, so no row ends before min_length tokens -- the
        local mask of the usual minimum-length processor, NOT conditioning on the length: it changes the measure that is sampled.
        None / 0 = off; with all three off the call runs exactly what it runs without them."""
        if min_p is not None or typical_p is not None or min_length != 0:
            if not sample:
                raise ValueError("min_p / typical_p / min_length need sample=True")
            return self._generate_trunc(conditions, max_length, temperature, early_stopping, use_graph, int(seed), top_k, top_p,
                                        min_p, typical_p, min_length)
        if top_k is not None or top_p is not None:
            if not sample:
                raise ValueError("top_k / top_p need sample=True")
            return self._generate_topkp(conditions, max_length, temperature, early_stopping, use_graph, int(seed), top_k, top_p)
        if sample:
            return self._generate_categorical(conditions, max_length, temperature, early_stopping, int(seed))
        dec = self.decoder
        ws, B = dec.load_conditions(conditions, max_length)
        st = self._state((B, max_length, float(temperature)), B, max_length)

        def enqueue():
            dec.dense_table(ws, mode=1, temperature=temperature)
            call("arcvae_dec_sample_chain", ptr(ws.nxt), ptr(st["tokens"]), ptr(st["first_end"]), B, dec.vocab_size,
                 max_length, dec.end_token, stream_ptr())

        _launch(st, enqueue, use_graph)
        return _stopped(st["tokens"], st["first_end"], early_stopping)

    def _state(self, key, B: int, T: int, more=None) -> dict:
        """self._graphs[key], made on the key's first use: the walk's output buffers, what else the pass keeps (`more()`) and the
        captured graph (None until _launch captures it)."""
        if key not in self._graphs:
            dev = self.decoder.store.device
            self._graphs[key] = dict(tokens=torch.zeros(B, T, dtype=torch.int32, device=dev),
                                     first_end=torch.zeros(B, dtype=torch.int32, device=dev), graph=None,
                                     **(more() if more else {}))
        return self._graphs[key]

    def _generate_categorical(self, conditions, max_length: int, temperature: float, early_stopping: bool, seed: int) -> torch.Tensor:
        """One dense decoder pass (raw logits of all B*V (row, token) pairs), then arcvae_dec_sample_chain_categorical: a wave per
        row walks start token -> sampled token -> ... through the table of distributions.  Eager launches (the seed is a launch
        argument; the greedy path's captured pass is untouched)."""
        check_temperature(temperature)
        dec = self.decoder
        ws, B = dec.load_conditions(conditions, max_length)
        tokens = torch.zeros(B, max_length, dtype=torch.int32, device=dec.store.device)
        first_end = torch.zeros(B, dtype=torch.int32, device=dec.store.device)
        dec.dense_table(ws)
        call("arcvae_dec_sample_chain_categorical", ptr(ws.logits), ptr(tokens), ptr(first_end), B, dec.vocab_size, max_length,
             dec.end_token, float(temperature), C.c_ulonglong(seed & 0xFFFFFFFFFFFFFFFF), stream_ptr())
        return _stopped(tokens, first_end, early_stopping)

    def _generate_topkp(self, conditions, max_length: int, temperature: float, early_stopping: bool, use_graph: bool, seed: int,
                        top_k, top_p) -> torch.Tensor:
        """One dense decoder pass (mode 0: raw logits of all B*V (row, token) pairs), then arcvae_dec_sample_chain_topkp: a pre-pass
        truncates every table row once, and a wave per row walks start token -> drawn token -> ... through those lists.  The seed is
        read by the kernel from a device word written before the launch, so the pass is captured once per (B, max_length,
        temperature, top_k, top_p) and replayed for every seed; use_graph=False launches the same kernels eagerly."""
        k, p = self._check_topkp(temperature, top_k, top_p)
        dec = self.decoder
        V = dec.vocab_size
        ws, B = dec.load_conditions(conditions, max_length)
        st = self._state(("topkp", B, max_length, float(temperature), k, p), B, max_length,
                         lambda: dict(seed=torch.zeros(1, dtype=torch.int64, device=dec.store.device),
                                      scratch=dec.scratch("topkp", B, V, k)))
        s64 = seed & 0xFFFFFFFFFFFFFFFF
        st["seed"].fill_(s64 - (1 << 64) if s64 >= 1 << 63 else s64)       # the 64-bit word the kernel reads

        def enqueue():
            dec.dense_table(ws)
            call("arcvae_dec_sample_chain_topkp", ptr(ws.logits), ptr(st["tokens"]), ptr(st["first_end"]), ptr(st["scratch"]),
                 st["scratch"].numel(), B, V, max_length, dec.end_token, float(temperature), k, p, ptr(st["seed"]), stream_ptr())

        _launch(st, enqueue, use_graph)
        return _stopped(st["tokens"], st["first_end"], early_stopping)

    def _check_topkp(self, temperature, top_k, top_p):
        """(k, p) as the kernels take them (0 / 1.0 = off), checked as the truncated walks need them."""
        check_temperature(temperature)
        k = 0 if top_k is None else int(top_k)
        if top_k is not None and k < 1:
            raise ValueError("top_k must be >= 1")
        p = 1.0 if top_p is None else float(top_p)
        if not 0.0 < p <= 1.0 or not 0.0 < float(C.c_float(p).value) <= 1.0:
            raise ValueError("top_p must lie in (0, 1]")
        if self.decoder.vocab_size > 256:
            raise ValueError("top-k / top-p sampling needs vocab_size <= 256")
        return k, p

    def _generate_trunc(self, conditions, max_length: int, temperature: float, early_stopping: bool, use_graph: bool, seed: int,
                        top_k, top_p, min_p, typical_p, min_length) -> torch.Tensor:
        """As _generate_topkp with arcvae_dec_sample_chain_trunc as the walk: the pre-pass writes the lists by the min-p or the
        typical rule, and with min_length > 0 a second set with the end token banned, which the steps t < min_length read.
        Captured once per (B, max_length, temperature, top_k, top_p, min_p, typical_p, min_length), replayed for every seed."""
        k, p, mp, tp, m = self._check_trunc(temperature, top_k, top_p, min_p, typical_p, min_length, max_length)
        dec = self.decoder
        V = dec.vocab_size
        ws, B = dec.load_conditions(conditions, max_length)
        st = self._state(("trunc", B, max_length, float(temperature), k, p, mp, tp, m), B, max_length,
                         lambda: dict(seed=torch.zeros(1, dtype=torch.int64, device=dec.store.device),
                                      scratch=dec.scratch("trunc", B, V, k, m)))
        s64 = seed & 0xFFFFFFFFFFFFFFFF
        st["seed"].fill_(s64 - (1 << 64) if s64 >= 1 << 63 else s64)       # the 64-bit word the kernel reads

        def enqueue():
            dec.dense_table(ws)
            call("arcvae_dec_sample_chain_trunc", ptr(ws.logits), ptr(st["tokens"]), ptr(st["first_end"]), ptr(st["scratch"]),
                 st["scratch"].numel(), B, V, max_length, m, dec.end_token, float(temperature), k, p, mp, tp, ptr(st["seed"]),
                 stream_ptr())

        _launch(st, enqueue, use_graph)
        return _stopped(st["tokens"], st["first_end"], early_stopping)

    def _check_trunc(self, temperature, top_k, top_p, min_p, typical_p, min_length, max_length):
        """(k, p, min_p, typical_p, min_length) as the list walks take them (0 / 1.0 / 0.0 / 1.0 / 0 = off), checked as
        arcvae_dec_sample_chain_trunc and arcvae_dec_sample_draws need them."""
        k, p = self._check_topkp(temperature, top_k, top_p)
        mp = 0.0 if min_p is None else float(min_p)
        if not 0.0 <= mp < 1.0 or not float(C.c_float(mp).value) < 1.0:
            raise ValueError("min_p must lie in [0, 1)")
        tp = 1.0 if typical_p is None else float(typical_p)
        if not 0.0 < tp <= 1.0 or not 0.0 < float(C.c_float(tp).value) <= 1.0:
            raise ValueError("typical_p must lie in (0, 1]")
        mp, tp = float(C.c_float(mp).value), float(C.c_float(tp).value)      # as the kernel receives them
        if tp < 1.0 and (p < 1.0 or mp > 0.0):
            raise ValueError("typical_p does not combine with top_p or min_p")
        V, m = self.decoder.vocab_size, int(min_length)
        if not 0 <= m <= int(max_length):
            raise ValueError("min_length must lie in [0, max_length]")
        if m > 0 and (V < 2 or not 0 <= self.decoder.end_token < V):
            raise ValueError("min_length needs vocab_size >= 2 and 0 <= end_token < vocab_size")
        return k, p, mp, tp, m

    def generate_many(self, conditions, num_draws: int, max_length: int = 80, temperature: float = 1.0, *, seed: int = 0,
                      top_k=None, top_p=None, min_p=None, typical_p=None, min_length: int = 0, early_stopping: bool = True,
                      use_graph: bool = True):
        """Extension (absent in the reference): num_draws INDEPENDENT random sequences per condition row -> (tokens [B, N, L]
        int32, lengths [B, N] int32).  The draws of a row are i.i.d. from exactly the measure the list walk of
        generate_with_temperature(sample=True, top_k / top_p / min_p / typical_p / min_length) samples -- with every rule off, the
        model's own distribution at this temperature -- and draw 0 is that call's molecule for the same seed.  Sampling WITH
        replacement: the same molecule may come twice; generate_without_replacement (num_samples) is the sampler of DISTINCT
        molecules, at most 32 per row and from another measure once truncation is wanted.
        For "N molecules at this property target" pass ONE condition row and num_draws = N, not N repeated rows: the dense table
        and its truncation are computed once per row of `conditions`, whatever num_draws is, and only the walk grows with it
        (include/arcvae_hip.h arcvae_dec_sample_draws: one thread per draw over the row's lists held in LDS).
        Tokens after a draw's first end_token are pad_token; lengths = the first end_token's index + 1, max_length without one.
        early_stopping: L = the longest draw; otherwise L = max_length.  The noise is keyed by (seed, row, draw, step): the same
        seed returns the same molecules, and the draws of a call are the first num_draws draws of any larger call.  The seed is
        read by the kernel from a device word, so the pass (dense table, pre-pass, walk) is captured once per (B, num_draws,
        max_length, temperature, top_k, top_p, min_p, typical_p, min_length) and replayed for every seed; use_graph=False launches
        the same kernels eagerly."""
        k, p, mp, tp, m = self._check_trunc(temperature, top_k, top_p, min_p, typical_p, min_length, max_length)
        N, T = int(num_draws), int(max_length)
        if N < 1:
            raise ValueError("num_draws must be >= 1")
        if not 0 <= self.pad_token <= 255:
            raise ValueError("needs 0 <= pad_token <= 255")
        dec = self.decoder
        V, dev = dec.vocab_size, dec.store.device
        ws, B = dec.load_conditions(conditions, T)
        if B * N > 2 ** 31 - 1 or B * (N + 255) > 2 ** 32 - 1:
            raise ValueError("need rows * num_draws <= 2**31 - 1 and rows * (num_draws + 255) <= 2**32 - 1")

        # the walk's buffers under _state's own names: tokens [B * N, T] and first_end [B * N] are [B, N, T] and [B, N] in memory
        st = self._state(("draws", B, N, T, float(temperature), k, p, mp, tp, m), B * N, T,
                         lambda: dict(seed=torch.zeros(1, dtype=torch.int64, device=dev),
                                      scratch=dec.scratch("sample_draws", B, V, k, m)))
        s64 = int(seed) & 0xFFFFFFFFFFFFFFFF
        st["seed"].fill_(s64 - (1 << 64) if s64 >= 1 << 63 else s64)       # the 64-bit word the kernel reads

        def enqueue():
            dec.dense_table(ws)
            call("arcvae_dec_sample_draws", ptr(ws.logits), ptr(st["tokens"]), ptr(st["first_end"]), ptr(st["scratch"]),
                 st["scratch"].numel(), B, N, V, T, m, dec.end_token, self.pad_token, float(temperature), k, p, mp, tp,
                 ptr(st["seed"]), stream_ptr())

        _launch(st, enqueue, use_graph)
        tokens, lengths = st["tokens"].view(B, N, T), torch.clamp(st["first_end"].view(B, N) + 1, max=T)
        return (_cut(tokens, lengths) if early_stopping else tokens).clone(), lengths

    def _check_lengths(self, max_length, min_length):
        """(max_length, min_length) as ints, checked as generate_beam, generate_map and generate_kbest need them."""
        T, m = int(max_length), int(min_length)
        if T < 1 or not 0 <= m <= T:
            raise ValueError("need max_length >= 1 and 0 <= min_length <= max_length")
        if not 0 <= self.pad_token <= 255:
            raise ValueError("needs 0 <= pad_token <= 255")
        return T, m

    def _check_chain(self, T: int, temperature) -> None:
        """What the kernels of csrc/chain.hip and csrc/kbest.hip refuse, as ValueErrors before any device work."""
        check_temperature(temperature, finite=True)
        if T < 1:
            raise ValueError("need max_length >= 1")
        if self.decoder.vocab_size > 256 or not 0 <= self.end_token < self.decoder.vocab_size:
            raise ValueError("needs vocab_size <= 256 and 0 <= end_token < vocab_size")

    def _length_divisors(self, length_penalty, T: int) -> torch.Tensor:
        """The [T] float32 device divisors of a length penalty (include/arcvae_hip.h len_div: entry n-1 divides the score of a
        sequence of n tokens), checked on the host before any device work.  A number alpha -> float(n) ** alpha in float64,
        rounded to float32 once (kept per (alpha, T) in self._divisors: the host loop and the copy to the device are paid once);
        a 1-D sequence / array / tensor of T numbers -> as given.  Every divisor must be finite and > 0 as a float32."""
        key = (length_penalty, T) if type(length_penalty) in (int, float) else None
        if key in self._divisors:
            return self._divisors[key]
        try:
            if isinstance(length_penalty, torch.Tensor):
                length_penalty = length_penalty.detach().cpu().numpy()
            a = np.asarray(length_penalty, dtype=np.float64)
            if a.ndim == 0:
                alpha = float(a)
                if not math.isfinite(alpha):
                    raise ValueError("length_penalty must be finite")
                a = np.array([float(n) ** alpha for n in range(1, T + 1)], dtype=np.float64)
        except (TypeError, ValueError, OverflowError) as e:
            raise ValueError(f"length_penalty: {e}") from None
        if a.shape != (T,):
            raise ValueError("length_penalty must be a number or max_length divisors")
        with np.errstate(over="ignore", under="ignore"):
            d = a.astype(np.float32)
        if not np.all(np.isfinite(d) & (d > 0)):
            raise ValueError("every length divisor must be finite and > 0 in float32")
        d = torch.as_tensor(d, device=self.decoder.store.device)
        if key is not None:
            self._divisors[key] = d
        return d

    def _table(self, conditions, T: int, temperature: float):
        """(ws, lse [B*V], B): the dense table of `conditions` in ws.logits (mode 0) and its rows' lse at `temperature`."""
        ws, B = self.decoder.load_conditions(conditions, T)
        self.decoder.dense_table(ws)
        return ws, self.decoder.table_lse(ws, temperature), B

    def _outputs(self, *shape):
        """(tokens [*lead, T] int32, scores [*lead] float32, lengths [*lead] int32) for shape = (*lead, T), uninitialised."""
        dev = self.decoder.store.device
        return (torch.empty(*shape, dtype=torch.int32, device=dev), torch.empty(*shape[:-1], dtype=torch.float32, device=dev),
                torch.empty(*shape[:-1], dtype=torch.int32, device=dev))

    def _profile(self, conditions, T: int, temperature: float):
        """One forward Viterbi pass that keeps the per-length profile -> (by_length [B, T], open_score [B], scratch, B): the best
        raw score of any sequence whose first end_token is at position t, the best score of one without, and the back pointers
        (include/arcvae_hip.h arcvae_dec_viterbi_norm, no divisors)."""
        self._check_lengths(T, 0)
        self._check_chain(T, temperature)
        V, dev = self.decoder.vocab_size, self.decoder.store.device
        ws, lse, B = self._table(conditions, T, temperature)
        scratch = self.decoder.scratch("viterbi", B, V, T)
        tokens, scores, lengths = self._outputs(B, T)
        raw, by_length, open_score = torch.empty_like(scores), torch.empty(B, T, dtype=torch.float32, device=dev), torch.empty_like(scores)
        call("arcvae_dec_viterbi_norm", ptr(ws.logits), ptr(lse), None, ptr(tokens), ptr(scores), ptr(raw), ptr(lengths),
             ptr(by_length), ptr(open_score), ptr(scratch), scratch.numel(), B, V, T, 0, self.end_token, self.pad_token,
             float(temperature), stream_ptr())
        return by_length, open_score, scratch, B

    def best_by_length(self, conditions, max_length: int = 80, temperature: float = 1.0):
        """Extension (absent in the reference): the best-molecule-per-length profile -> (scores [B, max_length] float32,
        open_score [B] float32).  scores[b, n-1] = the log-probability of the MOST PROBABLE sequence of exactly n tokens that ends
        with its first end_token there (-inf where there is none), exactly -- the e_t of the Viterbi recursion; open_score = the
        best sequence of max_length tokens without an end_token (-inf for a one-token vocabulary)."""
        by_length, open_score, _, _ = self._profile(conditions, int(max_length), temperature)
        return by_length, open_score

    def generate_of_length(self, conditions, lengths, max_length: int = 80, temperature: float = 1.0):
        """Extension (absent in the reference): the MOST PROBABLE sequence of exactly lengths[b] tokens (the end_token counts) per
        row -> (tokens [B, L] int32, L = the longest length asked for; scores [B] float32 = best_by_length at those lengths, equal to
        decoder.sequence_log_prob of the tokens bit for bit where finite).  lengths: an int, or a [B] sequence / tensor, entries in
        [1, max_length].  A score of -inf means no such sequence (the end token unreachable); its tokens are then arbitrary.  One
        forward pass and one back-trace (include/arcvae_hip.h arcvae_dec_viterbi_trace)."""
        T = int(max_length)
        if isinstance(lengths, torch.Tensor):
            lengths = lengths.detach().cpu().numpy()
        n = np.asarray(lengths)
        if n.dtype.kind not in "iu" or n.ndim > 1:
            raise ValueError("lengths must be an int or a [B] sequence of ints")
        if n.size == 0 or n.min() < 1 or n.max() > T:
            raise ValueError("need 1 <= lengths <= max_length")
        if n.ndim == 1 and n.shape[0] != len(conditions):
            raise ValueError("lengths must have one entry per row")
        by_length, _, scratch, B = self._profile(conditions, T, temperature)
        dev = self.decoder.store.device
        n_d = torch.as_tensor(np.broadcast_to(n, (B,)).astype(np.int32), device=dev)
        tokens = torch.empty(B, T, dtype=torch.int32, device=dev)
        call("arcvae_dec_viterbi_trace", ptr(scratch), scratch.numel(), ptr(n_d), ptr(tokens), B, self.decoder.vocab_size, T,
             self.end_token, self.pad_token, stream_ptr())
        scores = by_length.gather(1, (n_d.long() - 1)[:, None])[:, 0]
        return tokens[:, :int(n.max())].contiguous(), scores

    def generate_beam(self, z, conditions, max_length: int = 80, beam_width: int = 4, temperature: float = 1.0,
                      min_length: int = 0, early_stopping: bool = True):
        """Extension (absent in the reference): the beam_width most probable sequences per row under log_softmax(logits / T),
        found by beam search -> (tokens [B, K, L] int32, scores [B, K] float32, descending).  z is accepted and unused (Q2).
        Positions after a hypothesis' first end_token hold pad_token; end_token is not proposed before step min_length; ties
        are broken by parent slot, then token (the lower first).  A slot with no finite candidate (beam_width above what the
        vocabulary can fill) has score -inf and pad tokens.  early_stopping: L = the longest returned hypothesis (first EOS + 1,
        max_length without one); otherwise L = max_length.  Each score equals decoder.sequence_log_prob of its tokens."""
        V, K = self.decoder.vocab_size, int(beam_width)
        check_temperature(temperature)
        if not 1 <= K <= 32:
            raise ValueError("beam_width must lie in [1, 32]")
        T, min_length = self._check_lengths(max_length, min_length)
        if V > 256:
            raise ValueError("beam search needs vocab_size <= 256")
        ws, lse, B = self._table(conditions, T, temperature)
        scratch = self.decoder.scratch("beam", B, K, T)
        tokens, scores, lengths = self._outputs(B, K, T)
        call("arcvae_dec_beam_search", ptr(ws.logits), ptr(lse), ptr(tokens), ptr(scores), ptr(lengths), ptr(scratch),
             scratch.numel(), B, V, K, T, min_length, self.end_token, self.pad_token, float(temperature), stream_ptr())
        return (_cut(tokens, lengths).contiguous() if early_stopping else tokens), scores

    def generate_map(self, z, conditions, max_length: int = 80, temperature: float = 1.0, min_length: int = 0,
                     early_stopping: bool = True, length_penalty=None):
        """Extension (absent in the reference): the MOST PROBABLE sequence per row under log_softmax(logits / T), exactly -- a
        Viterbi recursion over the dense table (include/arcvae_hip.h arcvae_dec_viterbi) -> (tokens [B, L] int32, scores [B]
        float32).  z is accepted and unused (Q2).  A sequence ends with its first end_token, not before step min_length, or runs
        to max_length without one; positions after the end hold pad_token; ties go to the earliest end, then the lowest tokens.
        early_stopping: L = the longest returned sequence; otherwise L = max_length.  Each score equals
        decoder.sequence_log_prob of its tokens bit for bit, and is never below generate_beam's best at any width.
        length_penalty (None = the above, unchanged): a number alpha -> the sequence that maximises log-probability / n ** alpha
        over ALL admissible sequences, n its number of tokens (the end_token counts), exactly; or max_length divisors, entry n-1
        for length n.  Returns (tokens, scores, raw_scores): scores the normalised keys, raw_scores the log-probabilities
        (include/arcvae_hip.h arcvae_dec_viterbi_norm); key ties go to the earliest end."""
        T, min_length = self._check_lengths(max_length, min_length)
        self._check_chain(T, temperature)
        div = None if length_penalty is None else self._length_divisors(length_penalty, T)
        V = self.decoder.vocab_size
        ws, lse, B = self._table(conditions, T, temperature)
        scratch = self.decoder.scratch("viterbi", B, V, T)
        tokens, scores, lengths = self._outputs(B, T)
        if div is not None:
            raw = torch.empty_like(scores)
            call("arcvae_dec_viterbi_norm", ptr(ws.logits), ptr(lse), ptr(div), ptr(tokens), ptr(scores), ptr(raw), ptr(lengths),
                 None, None, ptr(scratch), scratch.numel(), B, V, T, min_length, self.end_token, self.pad_token, float(temperature),
                 stream_ptr())
            return (_cut(tokens, lengths).contiguous() if early_stopping else tokens), scores, raw
        call("arcvae_dec_viterbi", ptr(ws.logits), ptr(lse), ptr(tokens), ptr(scores), ptr(lengths), ptr(scratch), scratch.numel(),
             B, V, T, min_length, self.end_token, self.pad_token, float(temperature), stream_ptr())
        return (_cut(tokens, lengths).contiguous() if early_stopping else tokens), scores

    def generate_kbest(self, z, conditions, max_length: int = 80, num_best: int = 4, temperature: float = 1.0, min_length: int = 0,
                       early_stopping: bool = True, length_penalty=None):
        """Extension (absent in the reference): the num_best MOST PROBABLE sequences per row under log_softmax(logits / T), exactly
        -- a list-Viterbi recursion over the dense table (include/arcvae_hip.h arcvae_dec_kbest) -> (tokens [B, K, L] int32,
        scores [B, K] float32, descending).  z is accepted and unused (Q2).  Sequences, min_length and padding as in generate_map;
        the K sequences of a row are pairwise distinct, rank 0 is generate_map's, and no rank is below generate_beam's at
        beam_width = num_best.  A slot that no sequence fills (num_best above the number of admissible sequences) has score -inf
        and pad tokens.  early_stopping: L = the longest returned sequence (at least 1); otherwise L = max_length.  Each score
        equals decoder.sequence_log_prob of its tokens bit for bit; exp(scores).sum(1) is the probability mass the list covers.
        length_penalty (None = the above, unchanged; values as in generate_map): the K sequences with the largest normalised
        keys over all admissible sequences, exactly -> (tokens, scores, raw_scores), scores the keys, descending, raw_scores the
        log-probabilities (include/arcvae_hip.h arcvae_dec_kbest_norm); rank 0 is generate_map's under the same penalty."""
        K = int(num_best)
        if not 1 <= K <= 32:
            raise ValueError("num_best must lie in [1, 32]")
        T, min_length = self._check_lengths(max_length, min_length)
        self._check_chain(T, temperature)
        div = None if length_penalty is None else self._length_divisors(length_penalty, T)
        V = self.decoder.vocab_size
        ws, lse, B = self._table(conditions, T, temperature)
        scratch = self.decoder.scratch("kbest", B, V, K, T)
        tokens, scores, lengths = self._outputs(B, K, T)
        if div is not None:
            raw = torch.empty_like(scores)
            call("arcvae_dec_kbest_norm", ptr(ws.logits), ptr(lse), ptr(div), ptr(tokens), ptr(scores), ptr(raw), ptr(lengths),
                 ptr(scratch), scratch.numel(), B, V, K, T, min_length, self.end_token, self.pad_token, float(temperature),
                 stream_ptr())
            return (_cut(tokens, lengths, floor=1).contiguous() if early_stopping else tokens), scores, raw
        call("arcvae_dec_kbest", ptr(ws.logits), ptr(lse), ptr(tokens), ptr(scores), ptr(lengths), ptr(scratch), scratch.numel(),
             B, V, K, T, min_length, self.end_token, self.pad_token, float(temperature), stream_ptr())
        return (_cut(tokens, lengths, floor=1).contiguous() if early_stopping else tokens), scores

    def generate_without_replacement(self, z, conditions, max_length: int = 80, num_samples: int = 4, temperature: float = 1.0,
                                     seed: int = 0, early_stopping: bool = True, use_graph: bool = True, *,
                                     return_weights: bool = False):
        """Extension (absent in the reference): num_samples DISTINCT random sequences per row -- exactly a sample without
        replacement from the sequence distribution sample=True draws from at this temperature (stochastic beam search,
        include/arcvae_hip.h arcvae_dec_swor) -> (tokens [B, K, L] int32, log_probs [B, K] float32, perturbed [B, K] float32,
        descending, threshold [B] float32).  z is accepted and unused (Q2).  Rank 0 is one exact sample and does not depend on
        num_samples; the noise is keyed by (seed, row, token prefix): the same seed returns the same molecules.  Positions after
        a sequence's first end_token hold pad_token; a slot that no sequence fills (num_samples above the number of sequences) has
        log_probs = perturbed = -inf and pad tokens.  Each log_prob equals decoder.sequence_log_prob of its tokens bit for bit.
        threshold = the (K+1)-th largest perturbed value (-inf when nothing was left out).  perturbed and threshold are drawn
        given that the row's largest perturbed value is 0 (rank 0's is 0); `unconditioned` takes that conditioning out, and
        importance_weights(log_probs, unconditioned(threshold, seed)) are the inclusion-corrected weights.  return_weights=True
        appends weights [B, K]: the weights of the unbiased estimator sum_k weights[:, k] * f(x_k) of E_model[f(x)] -- the K-1
        highest ranks against the K-th sequence's unconditioned perturbed value, column K-1 zero (it needs num_samples >= 2).  early_stopping: L = the longest returned sequence (at least 1); otherwise L =
        max_length.  min_length, top_k / top_p and length penalties are not offered: each changes the measure that is sampled.
        The seed is read by the kernel from a device word written before the launch, so the pass (dense table, its lse, the walk)
        is captured once per (B, max_length, temperature, num_samples) and replayed for every seed; use_graph=False launches the
        same kernels eagerly."""
        K = int(num_samples)
        if not 1 <= K <= 32:
            raise ValueError("num_samples must lie in [1, 32]")
        T, _ = self._check_lengths(max_length, 0)
        self._check_chain(T, temperature)
        dec = self.decoder
        V, dev = dec.vocab_size, dec.store.device
        ws, B = dec.load_conditions(conditions, T)              # (the copy stays outside the captured pass, as in _table)

        def buffers():
            tokens, log_probs, lengths = self._outputs(B, K, T)
            return dict(seed=torch.zeros(1, dtype=torch.int64, device=dev), scratch=dec.scratch("swor", B, K, T),
                        lse=torch.empty(B * V, dtype=torch.float32, device=dev), out=tokens, log_probs=log_probs,
                        lengths=lengths, perturbed=torch.empty_like(log_probs),
                        threshold=torch.empty(B, dtype=torch.float32, device=dev))

        st = self._state(("swor", B, T, float(temperature), K), B, 1, buffers)
        s64 = int(seed) & 0xFFFFFFFFFFFFFFFF
        st["seed"].fill_(s64 - (1 << 64) if s64 >= 1 << 63 else s64)       # the 64-bit word the kernel reads

        def enqueue():
            dec.dense_table(ws)
            call("arcvae_dec_row_lse", ptr(ws.logits), ptr(st["lse"]), B * V, V, float(temperature), stream_ptr())
            call("arcvae_dec_swor", ptr(ws.logits), ptr(st["lse"]), ptr(st["seed"]), ptr(st["out"]), ptr(st["log_probs"]),
                 ptr(st["perturbed"]), ptr(st["lengths"]), ptr(st["threshold"]), ptr(st["scratch"]), st["scratch"].numel(), B, V, K,
                 T, self.end_token, self.pad_token, float(temperature), stream_ptr())

        _launch(st, enqueue, use_graph)
        tokens = (_cut(st["out"], st["lengths"], floor=1) if early_stopping else st["out"]).clone()
        log_probs, perturbed, threshold = st["log_probs"].clone(), st["perturbed"].clone(), st["threshold"].clone()
        if not return_weights:
            return tokens, log_probs, perturbed, threshold
        weights = importance_weights(log_probs, unconditioned(perturbed[:, K - 1], seed))
        weights[:, K - 1] = 0.0
        return tokens, log_probs, perturbed, threshold, weights

    def token_marginals(self, conditions, max_length: int = 80, temperature: float = 1.0) -> torch.Tensor:
        """Extension (absent in the reference): [B, max_length, V] float32, entry [b, t, v] = P(the token at step t is v and no
        end_token came before t) of what sample=True draws at this temperature -- the chain's forward recursion, exact up to fp32
        rounding (include/arcvae_hip.h arcvae_dec_chain_marginals).  Column end_token is the length distribution."""
        T, V = int(max_length), self.decoder.vocab_size
        self._check_chain(T, temperature)
        ws, lse, B = self._table(conditions, T, temperature)
        alive = torch.empty(B, T, V, dtype=torch.float32, device=self.decoder.store.device)
        call("arcvae_dec_chain_marginals", ptr(ws.logits), ptr(lse), ptr(alive), B, V, T, self.end_token, float(temperature),
             stream_ptr())
        return alive

    def length_distribution(self, conditions, max_length: int = 80, temperature: float = 1.0) -> torch.Tensor:
        """[B, max_length + 1] float32: entry t < max_length = P(length = t+1) (the end_token column of token_marginals), the
        last entry = P(no end_token within max_length), the mass a max_length cuts off."""
        alive = self.token_marginals(conditions, max_length, temperature)
        last = alive[:, -1, :]
        rest = last.sum(dim=1) - last[:, self.end_token]
        return torch.cat([alive[:, :, self.end_token], rest[:, None]], dim=1)

    def _expect(self, conditions, max_length, temperature, q=None, costs: bool = True, visits: bool = False):
        """The one path of the exact expectations -> (totals [B, n_cost] or None, visits [B, V] or None): the dense pass,
        arcvae_dec_row_lse, arcvae_dec_row_costs and arcvae_dec_chain_expect (include/arcvae_hip.h).  q = None: the row entropies
        alone (n_cost 1); q = (other_conditions, other, other_temperature), each None where Q does not differ from P there: the
        row cross-entropies against Q's table as well (n_cost 2).  The decoder's workspace is kept per (B, T), so a second dense
        pass on the same decoder overwrites ws.logits: P's table is then held in a copy of B * V * V * 4 bytes."""
        T, V, dev = int(max_length), self.decoder.vocab_size, self.decoder.store.device
        self._check_chain(T, temperature)
        if q is not None:
            other_conditions, other, other_temperature = q
            other = self if other is None else other
            temperature_q = temperature if other_temperature is None else other_temperature
            if not isinstance(other, MLXAutoregressiveDecoderSampling):
                raise ValueError("other must be a MLXAutoregressiveDecoderSampling")
            if other.decoder.vocab_size != V or other.end_token != self.end_token:
                raise ValueError("other must have the same vocab_size and end_token")
            other._check_chain(T, temperature_q)
            if other_conditions is not None and len(other_conditions) != len(conditions):
                raise ValueError("other_conditions must have one row per row of conditions")
        ws, lse, B = self._table(conditions, T, temperature)
        logits = ws.logits
        cost = totals = counts = None
        n_cost = 0
        if costs and q is None:
            n_cost = 1
            cost = torch.empty(1, B * V, dtype=torch.float32, device=dev)
            call("arcvae_dec_row_costs", ptr(logits), ptr(lse), float(temperature), None, None, float(temperature), ptr(cost),
                 None, B * V, V, stream_ptr())
        elif costs:
            n_cost = 2
            cost = torch.empty(2, B * V, dtype=torch.float32, device=dev)
            if other_conditions is None and other.decoder is self.decoder:      # the same table, at most another temperature
                logits_q = logits
                lse_q = lse if float(temperature_q) == float(temperature) else self.decoder.table_lse(ws, temperature_q)
            else:
                if other.decoder is self.decoder:
                    logits = logits.clone()                                      # (the second pass overwrites ws.logits)
                ws_q, lse_q, _ = other._table(conditions if other_conditions is None else other_conditions, T, temperature_q)
                logits_q = ws_q.logits
            call("arcvae_dec_row_costs", ptr(logits), ptr(lse), float(temperature), ptr(logits_q), ptr(lse_q), float(temperature_q),
                 ptr(cost[0]), ptr(cost[1]), B * V, V, stream_ptr())
        if n_cost:
            totals = torch.empty(B, n_cost, dtype=torch.float32, device=dev)
        if visits:
            counts = torch.empty(B, V, dtype=torch.float32, device=dev)
        call("arcvae_dec_chain_expect", ptr(logits), ptr(lse), ptr(cost), n_cost, ptr(totals), ptr(counts), None, B, V, T,
             self.end_token, float(temperature), stream_ptr())
        return totals, counts

    def sequence_entropy(self, conditions, max_length: int = 80, temperature: float = 1.0) -> torch.Tensor:
        """Extension (absent in the reference): [B] float32, the entropy in nats of the distribution over whole molecules that
        sample=True draws from at this temperature -- over the OUTCOMES of a row: a sequence up to and including its first
        end_token, or max_length tokens without one.  Exact up to fp32 rounding, nothing is sampled: by the chain rule it is the
        expected sum of the fed states' row entropies, a closed form on the forward recursion of token_marginals
        (include/arcvae_hip.h arcvae_dec_row_costs, arcvae_dec_chain_expect)."""
        totals, _ = self._expect(conditions, max_length, temperature)
        return totals[:, 0].contiguous()

    def expected_token_counts(self, conditions, max_length: int = 80, temperature: float = 1.0) -> torch.Tensor:
        """Extension (absent in the reference): [B, V] float32, entry [b, v] = the expected number of times token v is emitted
        in an outcome (token_marginals summed over the steps, without writing it).  Column end_token = P(the molecule ends
        within max_length)."""
        _, counts = self._expect(conditions, max_length, temperature, costs=False, visits=True)
        return counts

    def expected_length(self, conditions, max_length: int = 80, temperature: float = 1.0) -> torch.Tensor:
        """Extension (absent in the reference): [B] float32, the expected number of tokens of an outcome, the end_token counted
        and an outcome without one counting max_length: expected_token_counts summed over the tokens."""
        return self.expected_token_counts(conditions, max_length, temperature).sum(dim=1)

    def sequence_divergence(self, conditions, other_conditions=None, other=None, other_temperature=None, max_length: int = 80,
                            temperature: float = 1.0):
        """Extension (absent in the reference): (kl, cross_entropy, entropy), each [B] float32 in nats, between the outcome
        distribution P of (self, conditions, temperature) and a second one Q, paired row by row and both cut at max_length:
        entropy = sequence_entropy, cross_entropy = -E_P[log Q], kl = KL(P || Q) = cross_entropy - entropy, exactly (up to fp32
        rounding; nothing is sampled).  Q differs from P in any of: its conditions (other_conditions, as many rows), its
        temperature (other_temperature), its sampler (other: another MLXAutoregressiveDecoderSampling with the same vocab_size and
        end_token, e.g. one loaded with load_from_decoder(decoder, ema=...)); None = as P.  With nothing given Q = P and kl is
        exactly 0.  kl is not clamped: rounding may leave it slightly negative where P and Q nearly agree.  A token P emits and Q
        cannot gives +inf.  Cost: a second dense pass where the conditions or the sampler differ, and, when that pass runs on
        this sampler's own decoder, a copy of P's table, B * V * V * 4 bytes."""
        totals, _ = self._expect(conditions, max_length, temperature, q=(other_conditions, other, other_temperature))
        entropy, cross = totals[:, 0].contiguous(), totals[:, 1].contiguous()
        return cross - entropy, cross, entropy


def importance_weights(log_probs: torch.Tensor, threshold: torch.Tensor) -> torch.Tensor:
    """The weights exp(log_probs) / q of sequences sampled WITHOUT replacement (generate_without_replacement), [B, K] like
    log_probs: q = -expm1(-exp(log_probs - threshold[:, None])) is the probability that a sequence's perturbed value exceeds
    `threshold` [B].  exp(log_probs) where threshold is -inf (every sequence is included: q = 1); 0 for unfilled slots (log_probs
    -inf).  With threshold = the K-th sequence's UNCONDITIONED perturbed value (`unconditioned`), sum_k w_k f(x_k) over the K-1
    highest-ranked sequences is an UNBIASED estimator of E_model[f(x)] (Kool et al. 2019, section 4.2); these are the weights
    generate_without_replacement(return_weights=True) returns.  The values the walk returns are conditioned on the row's largest
    being 0; used as they are they give weights that are too small (the sum of the weights then averages E[(K-1) / (1 + Gamma(K-1))]
    instead of 1).  Evaluated in float64, returned in log_probs' dtype."""
    lp, thr = log_probs.double(), threshold.double()[:, None]
    e = torch.exp(lp - thr)                                     # (+inf at threshold -inf: q = 1)
    q = -torch.expm1(-e)
    w = torch.where(q > 0, torch.exp(lp) / q, torch.exp(thr).expand_as(lp))      # e underflows: exp(lp) / q -> exp(threshold)
    return torch.where(torch.isneginf(lp), torch.zeros_like(w), w).to(log_probs.dtype)


def _mix64(x: np.ndarray) -> np.ndarray:
    """splitmix64 finaliser (csrc/common.h mix64) on a uint64 array."""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def unconditioned(values: torch.Tensor, seed: int) -> torch.Tensor:
    """Perturbed values or thresholds of generate_without_replacement ([B] or [B, K], row b of the batch first) with the
    conditioning on the row's maximum taken out.  The walk starts every row at G = 0, i.e. it draws the perturbed values GIVEN that
    the largest of the row is 0: that leaves the sample and its order exact, but the estimator of importance_weights needs the
    values themselves.  As arrival times exp(-G) of a Poisson process the conditioning is a shift of the first arrival, so
    exp(-G') = exp(-G) - 1 + E with E ~ Exp(1) the row's largest value's own time: here E = -log(u) from the hash of the row's
    empty prefix, u = ((mix64(mix64(seed ^ (b << 32))) >> 40) + 0.5) * 2^-24 -- noise no sequence uses, a function of (seed, row).
    Monotone: the order, and -inf, are kept.  float64 inside, returned in values' dtype."""
    B = values.shape[0]
    h = _mix64(_mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ (np.arange(B, dtype=np.uint64) << np.uint64(32))))
    E = -np.log(((h >> np.uint64(40)).astype(np.float64) + 0.5) * 2.0 ** -24)
    E = torch.as_tensor(E, device=values.device).reshape((B,) + (1,) * (values.dim() - 1))
    return (-torch.log(torch.expm1(-values.double()) + E)).to(values.dtype)


def _launch(st: dict, enqueue, use_graph: bool) -> None:
    """Run `enqueue` (launches only: what it reads is written before) for the state `st` of one key: eagerly without use_graph;
    on the key's first use eagerly, then once more under capture; afterwards as a replay, which launches nothing from Python."""
    if not use_graph:
        enqueue()
    elif st["graph"] is None:
        enqueue()  # first call runs eagerly, then the decode pass is captured for replay
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            enqueue()
        st["graph"] = g
    else:
        st["graph"].replay()


def _cut(tokens: torch.Tensor, lengths: torch.Tensor, floor: int = 0, extra: int = 0) -> torch.Tensor:
    """Early stopping: the leading max(lengths) + extra columns of tokens [..., T], at least `floor` of them (a view; one host
    read of the device maximum replaces a per-step check)."""
    return tokens[..., :max(int(lengths.max().item()) + extra, floor)]


def _stopped(tokens: torch.Tensor, first_end: torch.Tensor, early_stopping: bool) -> torch.Tensor:
    """What a walk returns, as a copy of its buffer.  Early stopping as in the reference: its loop breaks at the first step where
    every row has already ended, i.e. after max_b(first EOS index) + 1 tokens."""
    return (_cut(tokens, first_end, extra=1) if early_stopping else tokens).clone()
