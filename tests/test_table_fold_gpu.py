"""arcvae_table_fold (csrc/misc.hip table_fold_kernel) against plain float64 numpy: the token-table fold on the exact-f32
MFMA forms with one owner per output element.

  dEmb += dT . Wx0[:, :E];   dWx0[:, :E] += dT^T . emb  (row stride E + C);   db0 += colsum(dT)

Shapes are those of test_kernels_gpu.py::test_table_finalize (ragged 16 x 16 and 32 x 32 tiles, E above 128, odd V: a
half-filled last K pair of the dWx0 product), the bar is that file's TOL."""
import numpy as np
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5          # tests/test_kernels_gpu.py TOL
SHAPES = [(80, 128, 0, 1024), (80, 128, 1, 1024), (95, 20, 2, 256), (33, 130, 3, 512), (127, 18, 0, 256)]


def _dev(a):
    return torch.tensor(a, dtype=torch.float32, device="cuda")


def _case(V, E, C, G):
    rs = np.random.RandomState(V + E)
    h = dict(dT=rs.standard_normal((V, G)), dT2=rs.standard_normal((V, G)), Wx0=rs.standard_normal((G, E + C)),
             emb=rs.standard_normal((V, E)), dEmb=rs.standard_normal((V, E)), dWx0=rs.standard_normal((G, E + C)),
             db0=rs.standard_normal(G))
    return {k: v.astype(np.float32) for k, v in h.items()}     # (the references below start from what the device holds)


def _fold(d, V, E, C, G, two=False, g_lo=0, g_hi=0, ldw=None):
    from arcvae_hip import _lib
    _lib.call("arcvae_table_fold", _lib.ptr(d["dT"]), _lib.ptr(d["dT2"] if two else None), _lib.ptr(d["Wx0"]),
              E + C if ldw is None else ldw, _lib.ptr(d["emb"]), _lib.ptr(d["dEmb"]), _lib.ptr(d["dWx0"]), _lib.ptr(d["db0"]),
              V, E, G, g_lo, g_hi, _lib.stream_ptr())
    torch.cuda.synchronize()


def _want(h, E, table):
    t = table.astype(np.float64)
    dWx0 = h["dWx0"].astype(np.float64)
    dWx0[:, :E] += t.T @ h["emb"].astype(np.float64)
    return h["dEmb"].astype(np.float64) + t @ h["Wx0"][:, :E].astype(np.float64), dWx0, h["db0"].astype(np.float64) + t.sum(0)


@pytest.mark.parametrize("V,E,C,G", SHAPES)
def test_fold_accumulates_onto_random_gradients(V, E, C, G):
    h = _case(V, E, C, G)
    d = {k: _dev(v) for k, v in h.items()}
    _fold(d, V, E, C, G)
    dEmb, dWx0, db0 = _want(h, E, h["dT"])
    got = d["dWx0"].cpu().numpy()
    for name, a, b in (("dEmb", d["dEmb"].cpu().numpy(), dEmb), ("dWx0", got, dWx0), ("db0", d["db0"].cpu().numpy(), db0)):
        print(f"V={V} E={E} C={C} G={G} {name}: rel_err {rel_err(a, b):.2e}")
        assert rel_err(a, b) < TOL, name
    assert np.array_equal(got[:, E:], h["dWx0"][:, E:])          # columns E .. E+C-1: not a bit touched
    for k in ("dT", "Wx0", "emb"):
        assert np.array_equal(d[k].cpu().numpy(), h[k]), k        # inputs are inputs


@pytest.mark.parametrize("V,E,C,G", SHAPES)
def test_second_table_is_summed_on_load(V, E, C, G):
    h = _case(V, E, C, G)
    d = {k: _dev(v) for k, v in h.items()}
    _fold(d, V, E, C, G, two=True)
    dEmb, dWx0, db0 = _want(h, E, h["dT"].astype(np.float64) + h["dT2"].astype(np.float64))
    assert rel_err(d["dEmb"].cpu().numpy(), dEmb) < TOL
    assert rel_err(d["dWx0"].cpu().numpy(), dWx0) < TOL
    assert rel_err(d["db0"].cpu().numpy(), db0) < TOL
    assert np.array_equal(d["dWx0"].cpu().numpy()[:, E:], h["dWx0"][:, E:])


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("V,E,C,G", SHAPES)
def test_dead_range_is_neither_read_nor_written(V, E, C, G, two):
    """Columns [G/4, G/2) of the table (the decoder's forget quarter) hold NaN: nothing of them may reach an output, and
    those rows of dWx0 / db0 keep their bits."""
    lo, hi = G // 4, G // 2
    h = _case(V, E, C, G)
    live = h["dT"].astype(np.float64) + (h["dT2"].astype(np.float64) if two else 0.0)
    live[:, lo:hi] = 0.0
    h["dT"][:, lo:hi] = np.nan
    h["dT2"][:, lo:hi] = np.nan
    d = {k: _dev(v) for k, v in h.items()}
    _fold(d, V, E, C, G, two=two, g_lo=lo, g_hi=hi)
    dEmb, dWx0, db0 = _want(h, E, live)
    got_e, got_w, got_b = d["dEmb"].cpu().numpy(), d["dWx0"].cpu().numpy(), d["db0"].cpu().numpy()
    assert np.isfinite(got_e).all() and np.isfinite(got_w).all() and np.isfinite(got_b).all()
    assert rel_err(got_e, dEmb) < TOL and rel_err(got_w, dWx0) < TOL and rel_err(got_b, db0) < TOL
    assert np.array_equal(got_w[lo:hi], h["dWx0"][lo:hi]) and np.array_equal(got_b[lo:hi], h["db0"][lo:hi])
    assert np.array_equal(got_w[:, E:], h["dWx0"][:, E:])


@pytest.mark.parametrize("V,E,C,G", SHAPES)
def test_two_runs_are_bit_identical(V, E, C, G):
    h = _case(V, E, C, G)
    outs = []
    for _ in range(2):
        d = {k: _dev(v) for k, v in h.items()}
        _fold(d, V, E, C, G, two=True, g_lo=G // 4, g_hi=G // 2)
        outs.append([d[k].cpu().numpy() for k in ("dEmb", "dWx0", "db0")])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_argument_errors():
    from arcvae_hip import _lib
    V, E, C, G = 95, 20, 2, 256
    h = _case(V, E, C, G)
    d = {k: _dev(v) for k, v in h.items()}
    before = {k: d[k].clone() for k in ("dEmb", "dWx0", "db0")}
    with pytest.raises(_lib.ArcvaeHipError):
        _fold(d, V, E, C, G, ldw=E - 1)
    for lo, hi in ((G // 4 + 16, G // 2), (G // 4, G // 2 + 8), (G // 2, G // 4), (0, G + 32), (-32, 32)):
        with pytest.raises(_lib.ArcvaeHipError):                  # the dead range lives on the kernel's 32-column grid, inside [0, G]
            _fold(d, V, E, C, G, g_lo=lo, g_hi=hi)
    with pytest.raises(_lib.ArcvaeHipError):
        _lib.call("arcvae_table_fold", _lib.ptr(d["dT"]), None, _lib.ptr(d["Wx0"]), E + C, _lib.ptr(d["emb"]), None,
                  _lib.ptr(d["dWx0"]), _lib.ptr(d["db0"]), V, E, G, 0, 0, _lib.stream_ptr())
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(d[k], t), k                            # a refused call launches nothing


@pytest.mark.parametrize("V,E,C,G", SHAPES)
def test_single_owner_outputs_equal_the_old_fold_bit_for_bit(V, E, C, G):
    """dWx0[:, :E] and db0 have one contribution per element in arcvae_table_finalize too (one atomic each), formed over the table
    rows in ascending order; the exact-f32 MFMA is an fmaf chain in that order and db0 is summed in that order: same bits.
    (dEmb is a sum of K slices in either kernel, in another order: compared through fp64 above.)"""
    from arcvae_hip import _lib
    h = _case(V, E, C, G)
    new = {k: _dev(v) for k, v in h.items()}
    old = {k: _dev(v) for k, v in h.items()}
    _fold(new, V, E, C, G)
    _lib.call("arcvae_table_finalize", _lib.ptr(old["dT"]), _lib.ptr(old["Wx0"]), E + C, _lib.ptr(old["emb"]), _lib.ptr(old["dEmb"]),
              _lib.ptr(old["dWx0"]), _lib.ptr(old["db0"]), V, E, G, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(new["db0"], old["db0"])
    assert torch.equal(new["dWx0"], old["dWx0"])
