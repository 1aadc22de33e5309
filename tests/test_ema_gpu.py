"""The weight EMA on the device (csrc/ema.hip, arcvae_hip/ema.py, trainer.py): the update kernel against the NumPy restatement
(tests/ema_ref.py) bit for bit, the guards, the exact swap, graph capture, and the update in its place -- behind every Adam
update of real training steps (single process with and without a predictor, two ranks), `applied()`, the sampler, and the
checkpoint round trip.  Nothing runs at the workload's size: the largest buffer is 100 003 floats."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch

import arcvae_oracle as O
import ema_ref as R
from helpers import HYPER, TINY, bits, rel_err

pytestmark = pytest.mark.gpu

B, T, LR, DECAY = 8, 12, 1e-2, 0.9
NULL = C.c_void_p(0)


# ---- raw launches -----------------------------------------------------------------------------------------------------
def _buf(values: np.ndarray, offset: int) -> torch.Tensor:
    """A device copy of `values` that starts `offset` floats behind a 16-byte boundary."""
    base = torch.empty(values.size + 4, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 16 == 0
    view = base[offset:offset + values.size]
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() % 16 == 4 * offset
    return view


def _launch(name, a, b, *tail):
    from arcvae_hip._lib import call, ptr_array, stream_ptr
    pa, keep_a = ptr_array(a)
    pb, keep_b = ptr_array(b)
    n = (C.c_long * len(a))(*[int(t.numel()) for t in a])
    call(name, pa, pb, n, len(a), *tail, stream_ptr())


def _update(e, p, omd, ga=NULL, gb=NULL):
    _launch("arcvae_ema_update", e, p, float(omd), ga, gb)


def _swap(a, b):
    _launch("arcvae_ema_swap", a, b)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _rand(n, seed):
    return np.random.RandomState(seed).standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("offsets", [(0, 0), (1, 1), (1, 0)], ids=["aligned", "offset", "mixed"])
@pytest.mark.parametrize("n", [1, 5, 1024, 100_003])
def test_update_matches_the_restatement_bit_for_bit(n, offsets):
    for omd in (0.1, 1e-4, 1.0):
        e0, p0 = _rand(n, 1), _rand(n, 2)
        e, p = _buf(e0, offsets[0]), _buf(p0, offsets[1])
        ref = e0
        for k in range(5):
            _update([e], [p], omd)
            ref = R.update32(ref, p0, R.omd32(omd))
            assert np.array_equal(bits(_np(e)), bits(ref)), (n, offsets, omd, k)
        assert np.array_equal(bits(_np(p)), bits(p0))          # params are never written
        if omd == 1.0:
            assert rel_err(_np(e), p0) <= 2.0 ** -22


def test_three_segments_in_one_launch():
    sizes, offs = (100_003, 7, 1024), (0, 1, 0)
    e0 = [_rand(n, 10 + i) for i, n in enumerate(sizes)]
    p0 = [_rand(n, 20 + i) for i, n in enumerate(sizes)]
    e = [_buf(v, o) for v, o in zip(e0, offs)]
    p = [_buf(v, o) for v, o in zip(p0, offs)]
    ref = list(e0)
    for k in range(5):
        omd = 1.0 - R.decay_at(0.999, True, k)
        _update(e, p, omd)
        ref = [R.update32(r, pp, R.omd32(omd)) for r, pp in zip(ref, p0)]
    for i in range(3):
        assert np.array_equal(bits(_np(e[i])), bits(ref[i])), i
        assert np.array_equal(bits(_np(p[i])), bits(p0[i])), i


def test_a_set_guard_word_leaves_every_shadow_untouched():
    sizes, offs = (4099, 7, 1024), (0, 1, 0)
    e0 = [_rand(n, 30 + i) for i, n in enumerate(sizes)]
    p0 = [_rand(n, 40 + i) for i, n in enumerate(sizes)]
    e = [_buf(v, o) for v, o in zip(e0, offs)]
    p = [_buf(v, o) for v, o in zip(p0, offs)]
    words = torch.zeros(64, dtype=torch.int32, device="cuda")
    ga, gb = C.c_void_p(words.data_ptr()), C.c_void_p(words.data_ptr() + 128)
    for set_a, set_b in ((1, 0), (0, 1), (7, 3)):
        words[0], words[32] = set_a, set_b
        _update(e, p, 0.25, ga, gb)
        if set_a:
            _update(e, p, 0.25, ga, NULL)                       # the set word alone, in either slot
            _update(e, p, 0.25, NULL, ga)
        if set_b:
            _update(e, p, 0.25, NULL, gb)
            _update(e, p, 0.25, gb, NULL)
        for i in range(3):
            assert np.array_equal(bits(_np(e[i])), bits(e0[i])), (set_a, set_b, i)
    words.zero_()
    _update(e, p, 0.25, ga, gb)                                 # zero words: the update runs
    for i in range(3):
        assert np.array_equal(bits(_np(e[i])), bits(R.update32(e0[i], p0[i], R.omd32(0.25)))), i


def test_swap_is_an_exact_exchange_and_its_own_inverse():
    sizes, offs_a, offs_b = (100_003, 7, 1024), (0, 1, 0), (0, 1, 1)
    a0 = [_rand(n, 50 + i) for i, n in enumerate(sizes)]
    b0 = [_rand(n, 60 + i) for i, n in enumerate(sizes)]
    a0[0][:4] = np.array([0x7FC00001, 0xFFC12345, 0x00000001, 0x80000000], dtype=np.uint32).view(np.float32)   # NaN payloads, a denormal, -0
    a = [_buf(v, o) for v, o in zip(a0, offs_a)]
    b = [_buf(v, o) for v, o in zip(b0, offs_b)]
    _swap(a, b)
    for i in range(3):
        assert np.array_equal(bits(_np(a[i])), bits(b0[i])) and np.array_equal(bits(_np(b[i])), bits(a0[i])), i
    _swap(a, b)
    for i in range(3):
        assert np.array_equal(bits(_np(a[i])), bits(a0[i])) and np.array_equal(bits(_np(b[i])), bits(b0[i])), i


def test_a_captured_update_replays():
    n = 4099
    e0, p0 = _rand(n, 70), _rand(n, 71)
    e, p = _buf(e0, 0), _buf(p0, 0)
    eager = _buf(e0, 0)
    for _ in range(3):
        _update([eager], [p], 0.1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _update([e], [p], 0.1)
    torch.cuda.synchronize()
    assert np.array_equal(bits(_np(e)), bits(e0))               # capturing runs nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(_np(e)), bits(_np(eager)))


# ---- the trainer ------------------------------------------------------------------------------------------------------
def _model(predictor_hidden: int = 0):
    from models.vae import ARCVAE
    cfg = TINY
    vae = ARCVAE(cfg.V, cfg.E, cfg.H, cfg.Z, cfg.C, cfg.L)
    params = O.init_params(cfg, 1234)
    vae.encoder.load_state_dict(params, prefix="encoder.")
    vae.decoder.load_state_dict(params, prefix="decoder.")
    pred = None
    if predictor_hidden:
        from models.property_predictor import PropertyPredictor
        pred = PropertyPredictor(cfg.Z, cfg.C, predictor_hidden, generator=torch.Generator().manual_seed(5))
    return vae, pred


def _trainer(tmp, vae, pred=None, **kw):
    from trainer import ARCVAETrainerWithLoss
    args = dict(learning_rate=LR, batch_size=B, lambda_collapse=0.001, free_bits=1.0, lambda_mi=0.01, progress=False,
                checkpoint_dir=str(tmp), ema_decay=DECAY, ema_warmup=True)
    args.update(kw)
    return ARCVAETrainerWithLoss(vae.encoder, vae.decoder, pred, None, **args)


def _stores(trainer):
    return {tag: mod.store for tag, mod in trainer._modules()}


def _steps(trainer, count, seed=100):
    """`count` training steps on seeded batches -> the weights of every store read back after each step."""
    hyper = trainer._hyper(0.05)
    after = []
    for k in range(count):
        x, cond = O.synthetic_batch(TINY, B, T, seed + k)
        np.random.seed(seed + k)
        trainer._train_step(x, cond, 0.7, hyper)
        torch.cuda.synchronize()
        after.append({tag: _np(st.flat) for tag, st in _stores(trainer).items()})
    return after


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """Six steps of an EMA trainer (shared, read-only): (vae, trainer, initial weights, weights after each step)."""
    vae, _ = _model()
    trainer = _trainer(tmp_path_factory.mktemp("ema"), vae)
    init = {tag: _np(st.flat) for tag, st in _stores(trainer).items()}
    after = _steps(trainer, 6)
    return vae, trainer, init, after


@pytest.mark.parametrize("predictor_hidden", [0, 16], ids=["pair", "with_predictor"])
def test_the_update_follows_every_adam_update_of_a_real_step(tmp_path, predictor_hidden):
    vae, pred = _model(predictor_hidden)
    trainer = _trainer(tmp_path, vae, pred)
    ema = trainer.ema
    tags = ["encoder", "decoder"] + (["predictor"] if pred is not None else [])
    assert list(ema.stores) == tags and ema.num_updates == 0
    ref = {tag: _np(st.flat) for tag, st in _stores(trainer).items()}
    for tag in tags:
        assert np.array_equal(bits(_np(ema.shadow(tag))), bits(ref[tag]))      # the shadow starts as a copy
    hyper = trainer._hyper(0.05)
    prev = dict(ref)
    for k in range(6):
        x, cond = O.synthetic_batch(TINY, B, T, 100 + k)
        np.random.seed(100 + k)
        trainer._train_step(x, cond, 0.7, hyper)
        torch.cuda.synchronize()
        omd = R.omd32(1.0 - R.decay_at(DECAY, True, k))
        for tag, st in _stores(trainer).items():
            p = _np(st.flat)
            assert not np.array_equal(bits(p), bits(prev[tag])), (k, tag)      # the step moved the weights
            prev[tag] = p
            ref[tag] = R.update32(ref[tag], p, omd)                            # ... and the EMA read the MOVED ones
            assert np.array_equal(bits(_np(ema.shadow(tag))), bits(ref[tag])), (k, tag)
    assert ema.num_updates == 6
    trainer.engine.check_gates()
    before = {tag: _np(st.flat) for tag, st in _stores(trainer).items()}
    ema.update()
    torch.cuda.synchronize()
    assert ema.num_updates == 7
    for tag, st in _stores(trainer).items():
        assert np.array_equal(bits(_np(st.flat)), bits(before[tag])), tag      # update() never writes the weights
        assert np.array_equal(bits(_np(ema.shadow(tag))),
                              bits(R.update32(ref[tag], before[tag], R.omd32(1.0 - R.decay_at(DECAY, True, 6))))), tag


def test_trained_fixture_matches_the_replay(trained):
    _vae, trainer, init, after = trained
    for tag in ("encoder", "decoder"):
        ref = R.replay(init[tag], [a[tag] for a in after], DECAY, True)
        assert np.array_equal(bits(_np(trainer.ema.shadow(tag))), bits(ref)), tag
    assert trainer.ema.num_updates == 6


def _loss_vector(encoder, decoder, x, cond, eps):
    from arcvae_hip import api
    out = api.loss_forward(encoder, decoder, x, cond, eps=eps, coins=np.zeros(T, dtype=np.uint8), **HYPER)
    torch.cuda.synchronize()
    return np.array([float(out[k]) for k in ("total_loss", "recon_loss", "kl_loss")]), _np(out["mu"])


def test_applied_exchanges_weights_and_shadow(trained):
    vae, trainer, _init, _after = trained
    ema = trainer.ema
    stores = _stores(trainer)
    raw = {tag: _np(st.flat) for tag, st in stores.items()}
    avg = {tag: _np(ema.shadow(tag)) for tag in stores}
    x, cond = O.synthetic_batch(TINY, B, T, 7)
    eps = torch.as_tensor(_rand(B * TINY.Z, 8).reshape(B, TINY.Z), device="cuda")

    fresh, _ = _model()
    fresh.encoder.store.flat.copy_(ema.shadow("encoder"))
    fresh.decoder.store.flat.copy_(ema.shadow("decoder"))
    want, want_mu = _loss_vector(fresh.encoder, fresh.decoder, x, cond, eps)
    raw_loss, _ = _loss_vector(vae.encoder, vae.decoder, x, cond, eps)
    print("loss on averaged weights", want, "on raw weights", raw_loss, "rel", rel_err(raw_loss, want))
    assert rel_err(raw_loss, want) > 10 * 1e-5          # otherwise the check below shows nothing

    with ema.applied():
        for tag, st in stores.items():
            assert np.array_equal(bits(_np(st.flat)), bits(avg[tag])), tag
            assert np.array_equal(bits(_np(ema.shadow(tag))), bits(raw[tag])), tag
        got, got_mu = _loss_vector(vae.encoder, vae.decoder, x, cond, eps)
        with pytest.raises(RuntimeError):
            ema.update()
        with pytest.raises(RuntimeError):
            with ema.applied():
                pass
    assert rel_err(got, want) <= 1e-5 and rel_err(got_mu, want_mu) <= 1e-5, (got, want)

    def restored():
        torch.cuda.synchronize()
        return all(np.array_equal(bits(_np(st.flat)), bits(raw[tag])) and
                   np.array_equal(bits(_np(ema.shadow(tag))), bits(avg[tag])) for tag, st in stores.items())
    assert restored()
    with pytest.raises(KeyError):
        with ema.applied():
            raise KeyError("inside")
    assert restored() and ema.num_updates == 6
    again, _ = _loss_vector(vae.encoder, vae.decoder, x, cond, eps)
    assert rel_err(again, raw_loss) <= 1e-5


def test_sampler_loads_the_average(trained):
    vae, trainer, _init, _after = trained
    ema = trainer.ema
    cond = _rand(4 * TINY.C, 9).reshape(4, TINY.C)
    vae.decoder_sampling.load_from_decoder(vae.decoder, ema=ema)
    assert np.array_equal(bits(_np(vae.decoder_sampling.decoder.store.flat)), bits(_np(ema.shadow("decoder"))))
    got = _np(vae.generate(4, cond, max_length=12))
    with ema.applied():
        vae.decoder_sampling.load_from_decoder(vae.decoder)
    want = _np(vae.generate(4, cond, max_length=12))
    assert np.array_equal(got, want)
    other, _ = _model()
    with pytest.raises(ValueError):
        other.decoder_sampling.load_from_decoder(other.decoder, ema=ema)      # an EMA of another decoder


def test_checkpoint_round_trip(tmp_path):
    vae, _ = _model()
    trainer = _trainer(tmp_path / "a", vae)
    _steps(trainer, 3)
    saved = {}
    trainer._save_checkpoint = lambda ck, path: saved.update(ck)
    trainer.save_checkpoint(epoch=0)
    names = list(vae.encoder.store.names())
    assert "ema_json" in saved and all(f"encoder_ema_weights/{n}" in saved for n in names)
    assert all(f"decoder_ema_weights/{n}" in saved for n in vae.decoder.store.names())
    path = str(tmp_path / "ck.npz")
    np.savez(path, **saved)

    vae2, _ = _model()
    fresh = _trainer(tmp_path / "b", vae2)
    fresh.load_checkpoint(path)
    torch.cuda.synchronize()
    assert fresh.ema.num_updates == 3
    for tag in ("encoder", "decoder"):
        st = _stores(fresh)[tag]
        assert np.array_equal(bits(_np(st.flat)), bits(_np(_stores(trainer)[tag].flat))), tag
        assert np.array_equal(bits(_np(fresh.ema.shadow(tag))), bits(_np(trainer.ema.shadow(tag)))), tag
    before = {tag: _np(fresh.ema.shadow(tag)) for tag in ("encoder", "decoder")}
    fresh.ema.update()                                          # the fourth update: decay_at(3)
    torch.cuda.synchronize()
    omd = R.omd32(1.0 - R.decay_at(DECAY, True, 3))
    for tag in ("encoder", "decoder"):
        assert np.array_equal(bits(_np(fresh.ema.shadow(tag))), bits(R.update32(before[tag], _np(_stores(fresh)[tag].flat), omd))), tag

    # a checkpoint without an EMA: the average restarts from the loaded weights
    plain = {k: v for k, v in saved.items() if "ema" not in k}
    path2 = str(tmp_path / "plain.npz")
    np.savez(path2, **plain)
    vae3, _ = _model()
    third = _trainer(tmp_path / "c", vae3)
    third.ema.num_updates = 5
    third.load_checkpoint(path2)
    torch.cuda.synchronize()
    assert third.ema.num_updates == 0
    for tag in ("encoder", "decoder"):
        assert np.array_equal(bits(_np(third.ema.shadow(tag))), bits(_np(_stores(third)[tag].flat))), tag
        assert np.array_equal(bits(_np(_stores(third)[tag].flat)), bits(_np(_stores(trainer)[tag].flat))), tag
    # a trainer without an EMA ignores the extra keys
    vae4, _ = _model()
    off = _trainer(tmp_path / "d", vae4, ema_decay=None, ema_warmup=False)
    off.load_checkpoint(path)
    assert off.ema is None
    assert np.array_equal(bits(_np(vae4.decoder.store.flat)), bits(_np(vae.decoder.store.flat)))


# ---- two ranks on one GPU ---------------------------------------------------------------------------------------------
def _paths():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "mlx-vae_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, tmp, ret):
    _paths()
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from arcvae_hip import api
    vae, _ = _model()
    dp = api.enable_data_parallel(vae.encoder, vae.decoder)
    trainer = _trainer(os.path.join(tmp, f"r{rank}"), vae)
    assert (trainer.rank, trainer.world) == (rank, world) and dp.ema is trainer.ema
    init = {tag: _np(st.flat) for tag, st in _stores(trainer).items()}
    after = _steps(trainer, 3)
    # a batch with fewer rows than ranks is replicated and rank 0's state broadcast: the shadows travel with it -- shown on a
    # rank whose shadow was made to drift first
    if rank == 1:
        trainer.ema.shadow("decoder")[:16] += 1.0
    x1, cond1 = O.synthetic_batch(TINY, 1, T, 300)
    np.random.seed(300)
    trainer._train_step(x1, cond1, 0.7, trainer._hyper(0.05))
    torch.cuda.synchronize()
    after.append({tag: _np(st.flat) for tag, st in _stores(trainer).items()})
    trainer.engine.check_gates()
    ret[rank] = dict(init=init, after=after, shadow={tag: _np(trainer.ema.shadow(tag)) for tag in init},
                     num_updates=trainer.ema.num_updates)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_keep_identical_shadows(tmp_path):
    import torch.multiprocessing as mp
    _paths()
    os.makedirs(tmp_path / "dp", exist_ok=True)
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path / "dp"), ret), nprocs=world, join=True)
    r0, r1 = ret[0], ret[1]
    assert r0["num_updates"] == r1["num_updates"] == 4          # three sharded steps and the replicated one
    for tag in ("encoder", "decoder"):
        assert np.array_equal(bits(r0["shadow"][tag]), bits(r1["shadow"][tag])), tag
        ref = R.replay(r0["init"][tag], [a[tag] for a in r0["after"]], DECAY, True)
        assert np.array_equal(bits(r0["shadow"][tag]), bits(ref)), tag
