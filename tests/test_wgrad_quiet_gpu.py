"""The quiet split-bf16 TN "+=" kernel (csrc/gemm.hip wgrad_quiet_kernel: ARCVAE_GEMM_QUIET, arcvae_enc_lstm_wgrad parts
bit 9) against fp64: alone on the shapes at which its staging, ring and ragged edges can go wrong, grouped through the
weight-gradient entry point over the time ranges that give K = 0, one tick and unequal K in one launch, and in the
default-architecture training step beside the persistent BPTT sweep."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import DEFAULT, ELEM_ATOL_GRAD, HYPER, assert_elem, build_engine, elem_err, make_case, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _dev(a):
    return torch.tensor(a, dtype=torch.float32, device="cuda")


# (M, N, K, ldc_pad): one K step (less than the ring depth); ragged K; K one past 4096 with a padded C; the one-hot shape
# (ragged M); ragged N; smaller than one tile both ways
@pytest.mark.parametrize("M,N,K,ldc_pad", [(128, 128, 16, 0), (128, 128, 531, 0), (256, 256, 4097, 5), (80, 1024, 2000, 0),
                                           (1024, 40, 100, 0), (36, 72, 64, 0)])
def test_quiet_tn_gemm_has_f32_accuracy(M, N, K, ldc_pad):
    """Same operand recipe and criterion as test_split_bf16_tn_gemm_has_f32_accuracy: worst element error relative to
    sum |a||b| within 2x the exact-f32 kernel's on the same data (floor 2e-7), and the 1e-4 / 1e-6 element-wise parity
    criterion passed by a factor of five; padding columns of C bit-identical."""
    from arcvae_hip import _lib
    rs = np.random.RandomState(M + N + K)
    A = (rs.standard_normal((K, M)) * np.exp(rs.uniform(-3, 3, size=(K, 1)))).astype(np.float32)   # wide dynamic range
    Bm = rs.standard_normal((K, N)).astype(np.float32)
    ld = N + ldc_pad
    C0 = rs.standard_normal((M, ld)).astype(np.float32)
    ref = C0.astype(np.float64).copy()
    ref[:, :N] += A.T.astype(np.float64) @ Bm.astype(np.float64)
    mag = np.abs(A.T.astype(np.float64)) @ np.abs(Bm.astype(np.float64))       # sum |a||b| per element
    dA, dB = _dev(A), _dev(Bm)
    out, res = {}, {}
    for name, flags in (("quiet", _lib.GEMM_ACCUMULATE | _lib.GEMM_SPLITK | _lib.GEMM_QUIET), ("f32", _lib.GEMM_ACCUMULATE)):
        dC = _dev(C0)
        _lib.gemm(True, False, M, N, K, dA, M, dB, N, dC, ld, None, flags)
        torch.cuda.synchronize()
        res[name] = dC.cpu().numpy()
        got = res[name].astype(np.float64)
        if ldc_pad:
            assert np.array_equal(res[name][:, N:], C0[:, N:])   # padding columns untouched
        out[name] = np.abs(got[:, :N] - ref[:, :N]) / (mag + 1e-30)
    print(f"quiet {out['quiet'].max():.3e}  f32 {out['f32'].max():.3e}  elem {elem_err(res['quiet'][:, :N], ref[:, :N], 1e-4, 1e-6)[0]:.3e}")
    assert out["quiet"].max() <= max(2.0 * out["f32"].max(), 2e-7), (out["quiet"].max(), out["f32"].max())
    assert elem_err(res["quiet"][:, :N], ref[:, :N], 1e-4, 1e-6)[0] < 0.2


def test_quiet_flag_refuses_operands_it_cannot_stage():
    """No other kernel runs in its place: a B whose rows are not 16-byte aligned is an argument error."""
    from arcvae_hip import _lib
    M, N, K = 64, 62, 32
    dA, dB, dC = torch.zeros(K, M, device="cuda"), torch.zeros(K, N, device="cuda"), torch.zeros(M, N, device="cuda")
    rc = _lib.load().arcvae_gemm_f32(1, 0, M, N, K, _lib.ptr(dA), M, _lib.ptr(dB), N, _lib.ptr(dC), N, None,
                                     _lib.GEMM_ACCUMULATE | _lib.GEMM_SPLITK | _lib.GEMM_QUIET, _lib.stream_ptr())
    assert rc != 0


@pytest.fixture(scope="module")
def stack_case():
    """dG / hseq / tokens of an H 256, L 2, B 8, T 5 stack and their fp64 forms (shared by the ranges, never written)."""
    B, H, L, T, V, E = 8, 256, 2, 5, 80, 16
    rs = np.random.RandomState(29)
    hseq = rs.standard_normal((L, T, B, H)).astype(np.float32)
    dG = (rs.standard_normal((L, T, B, 4 * H)) * np.exp(rs.uniform(-2, 2, size=(L, T, B, 1)))).astype(np.float32)
    x = rs.randint(0, V, size=(T, B)).astype(np.int32)
    return dict(B=B, H=H, L=L, T=T, V=V, E=E, hseq=hseq, dG=dG, x=x, h64=hseq.astype(np.float64), g64=dG.astype(np.float64))


@pytest.mark.parametrize("t_lo,t_hi", [(0, 5), (0, 1), (1, 2), (3, 5)])
def test_grouped_weight_gradients_on_the_quiet_kernel(stack_case, t_lo, t_hi):
    """arcvae_enc_lstm_wgrad with parts bit 9, one launch per range: [0, 5) (dWh is B rows shorter than dWx: unequal K in
    one group), [0, 1) (dWh has K = 0: its problem is absent and dWh stays exactly 0), [1, 2) (one tick, K = B < one
    stage), [3, 5).  dWh_l, dWx_1, dbias_1 and the token table (its own, unchanged kernel) against fp64 contractions."""
    from arcvae_hip import _lib
    c = stack_case
    B, H, L, T, V, E = c["B"], c["H"], c["L"], c["T"], c["V"], c["E"]
    G = 4 * H
    hseq, dG = _dev(c["hseq"]), _dev(c["dG"])
    dWh = [torch.zeros(G, H, device="cuda") for _ in range(L)]
    dWx = [torch.zeros(G, E, device="cuda"), torch.zeros(G, H, device="cuda")]
    dbias = [torch.zeros(G, device="cuda") for _ in range(L)]
    x_tb = torch.tensor(c["x"], dtype=torch.int32, device="cuda")
    emb, wx0 = torch.zeros(V, E, device="cuda"), torch.zeros(G, E, device="cuda")
    dtab, onehot, demb = torch.full((V, G), 7.0, device="cuda"), torch.zeros(T * B, V, device="cuda"), torch.zeros(V, E, device="cuda")
    pwx, _a = _lib.ptr_array(dWx); pwh, _b = _lib.ptr_array(dWh); pbs, _c = _lib.ptr_array(dbias)
    rc = _lib.load().arcvae_enc_lstm_wgrad(_lib.ptr(x_tb), _lib.ptr(emb), _lib.ptr(wx0), _lib.ptr(hseq), _lib.ptr(dG),
                                           _lib.ptr(dtab), _lib.ptr(onehot), _lib.ptr(demb), pwx, pwh, pbs, B, T, V, E, H, L,
                                           t_lo, t_hi, 1, 0, 1 | 2 | _lib.WGRAD_QUIET, None, None, None, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    g64, h64 = c["g64"], c["h64"]

    def check(name, got, ref):
        got = got.cpu().numpy()
        if np.abs(ref).max() == 0.0:
            assert np.abs(got).max() == 0.0, name
            return
        print(f"[{t_lo},{t_hi}) {name}: rel {rel_err(got, ref):.3e} elem {elem_err(got, ref, 1e-4, 1e-6)[0]:.3e}")
        assert rel_err(got, ref) < TOL, name
        assert_elem(got, ref, name, 1e-6)

    for l in range(L):                                            # dWh_l = sum_t dG_l[t]^T h_l[t-1], t >= 1
        check(f"dWh_{l}", dWh[l], sum((g64[l, t].T @ h64[l, t - 1] for t in range(max(t_lo, 1), t_hi)), np.zeros((G, H))))
    check("dWx_1", dWx[1], sum(g64[1, t].T @ h64[0, t] for t in range(t_lo, t_hi)))
    check("dbias_1", dbias[1], g64[1, t_lo:t_hi].sum((0, 1)))
    assert np.abs(dbias[0].cpu().numpy()).max() == 0.0 and np.abs(dWx[0].cpu().numpy()).max() == 0.0   # layer 0: by the table
    tab = np.zeros((V, G))
    for t in range(t_lo, t_hi):
        np.add.at(tab, c["x"][t], g64[0, t])
    check("dtable", dtab, tab)


def _encoder_step(B, T):
    """One default-architecture step; every encoder gradient against the fp64 oracle (norm-wise and element-wise at 1e-4,
    dead parameters exactly 0)."""
    cfg = DEFAULT
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.9)
    import arcvae_oracle as O
    _vals, grads = O.loss_and_grads(params, cfg, x, cond, eps, coins, dtype=torch.float64, **HYPER)
    eng, enc, _dec = build_engine(cfg, params)
    eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, **HYPER)
    torch.cuda.synchronize()
    eng.check_gates()
    from arcvae_hip.engine import bptt_reduce_scatter_ok
    assert bptt_reduce_scatter_ok(eng.workspace(B, T), eng.d)      # the regime in which the kernel is selected
    n = 0
    for name, g in grads.items():
        mod, pname = name.split(".", 1)
        if mod != "encoder":
            continue
        got = enc.g(pname).cpu().numpy()
        if np.abs(g).max() == 0.0:
            assert np.abs(got).max() == 0.0, f"dead parameter {name} received gradient"
        else:
            assert rel_err(got, g) < TOL, (name, rel_err(got, g))
            assert_elem(got, g, "grad " + name, ELEM_ATOL_GRAD)
            n += 1
    assert n >= 8


@pytest.mark.parametrize("B", [8, 64])
def test_default_step_encoder_gradients_with_the_quiet_kernel(B, monkeypatch):
    monkeypatch.setenv("ARCVAE_WGRAD_QUIET", "1")
    _encoder_step(B, 6)


def test_default_step_encoder_gradients_with_the_switch_off(monkeypatch):
    """ARCVAE_WGRAD_QUIET=0 restores the LDS-free split kernel: the same step, the same bar."""
    monkeypatch.setenv("ARCVAE_WGRAD_QUIET", "0")
    _encoder_step(64, 6)
