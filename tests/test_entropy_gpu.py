"""Exact entropy, cross-entropy, KL, expected token counts and length of the molecule distribution on the GPU
(csrc/table.hip arcvae_dec_row_costs, csrc/chain.hip arcvae_dec_chain_expect; an extension with no reference behaviour to match):
the two kernels against the fp64 restatement (tests/entropy_ref.py) inside worst-case rounding bounds, and the model-level surface
(sequence_entropy, expected_token_counts, expected_length, sequence_divergence) against the same restatement on the decoder's own
tables."""
import numpy as np
import pytest
import torch

import beam_ref as R
import chain_ref as X
import entropy_ref as N
from helpers import dev as _dev, ending_model, lib as _lib

pytestmark = pytest.mark.gpu
U23, U24 = 2.0 ** -23, 2.0 ** -24


def _row_costs(tp, lp, temp_p, tq, lq, temp_q, R_, V):
    """h, c [R] (c None without q) as numpy, from device tensors."""
    L = _lib()
    h = torch.full((R_,), -7.0, dtype=torch.float32, device="cuda")
    c = None if tq is None else torch.full((R_,), -7.0, dtype=torch.float32, device="cuda")
    L.call("arcvae_dec_row_costs", L.ptr(tp), L.ptr(lp), float(temp_p), L.ptr(tq), L.ptr(lq), float(temp_q), L.ptr(h), L.ptr(c),
           R_, V, L.stream_ptr())
    return h, c


def _expect(tab, lse, cost, n_cost, B, V, T, end, temp, totals=True, visits=True, open_mass=True):
    """(totals [B, n_cost], visits [B, V], open_mass [B]) device tensors pre-filled with -7; an output not asked for keeps it."""
    L = _lib()
    to = torch.full((B, max(n_cost, 1)), -7.0, dtype=torch.float32, device="cuda")
    vi = torch.full((B, V), -7.0, dtype=torch.float32, device="cuda")
    om = torch.full((B,), -7.0, dtype=torch.float32, device="cuda")
    L.call("arcvae_dec_chain_expect", L.ptr(tab), L.ptr(lse), L.ptr(cost if totals else None), n_cost if totals else 0,
           L.ptr(to if totals else None), L.ptr(vi if visits else None), L.ptr(om if open_mass else None), B, V, T, end,
           float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    return to.cpu().numpy(), vi.cpu().numpy(), om.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# (V, max_len, temperature, end_token): no recursion; cont of one step and visits of two; two parts; the start row is the end
# token's row; staged in three parts; the largest staged V; read through L2 with V no multiple of 4; one part; V 256; V 1 (the
# only outcome is the end token at once: every total is exactly 0).
CASES = [(12, 1, 1.0, 2), (12, 2, 1.0, 2), (12, 16, 0.7, 2), (12, 8, 1.0, 0), (80, 24, 1.0, 2), (96, 5, 1.0, 2), (97, 5, 1.0, 5),
         (130, 4, 0.7, 2), (256, 8, 1.3, 2), (1, 4, 1.0, 0)]


@pytest.mark.parametrize("V,T,temp,end", CASES)
def test_kernels_against_fp64(V, T, temp, end):
    """The fp64 reference runs over the FP32 step terms (the same lse passed in), so only expf, the products and the sums
    differ.  Worst-case bounds, u = 2^-24: a row cost carries (V + 8) u of its absolute-term sum, alive T (V + 8) u, the running
    sum over the steps T u and the final sum over the columns (V + 2) u, all on non-negative magnitudes; doubled:
    |total - ref| <= (T + 2)(V + 8) 2^-23 A, A the reference's sum of absolute terms; |visits / ref - 1| and |open_mass / ref - 1|
    <= (T + 1)(V + 8) 2^-24; the KL's absolute tolerance is the sum of the two totals' bounds.
    Measured on an MI355X, worst |total - ref| / bound over these cases: see DESIGN.md section 10."""
    B, temp_q = 3, 2.0 * temp                                    # (V 1: x / 2 is exact, so lq is exactly 0 as lp is)
    rs = np.random.RandomState(V * 100 + T)
    tab_p, tab_q = X.make_table(rs, B, V, "normal", end), X.make_table(rs, B, V, "normal", end)
    lse_p, lse_q = R.row_lse(tab_p, temp).astype(np.float32), R.row_lse(tab_q, temp_q).astype(np.float32)
    tp, lp, tq, lq = (_dev(a, torch.float32) for a in (tab_p, lse_p, tab_q, lse_q))
    h, c = _row_costs(tp, lp, temp, tq, lq, temp_q, B * V, V)
    cost = torch.stack([h, c]).contiguous()
    totals, visits, open_mass = _expect(tp, lp, cost, 2, B, V, T, end, temp)
    ref = N.expectations(R.step_terms(tab_p, lse_p, temp), R.step_terms(tab_q, lse_q, temp_q), B, V, T, end)

    # the row costs themselves, inside their share of the bound
    for got, lq_terms in ((h, R.step_terms(tab_p, lse_p, temp)), (c, R.step_terms(tab_q, lse_q, temp_q))):
        r, a = N.row_costs(R.step_terms(tab_p, lse_p, temp), lq_terms)
        assert np.all(np.abs(got.cpu().numpy() - r) <= 2 * (V + 8) * U24 * a)

    tot = totals.astype(np.float64)
    bound_h, bound_ce = (T + 2) * (V + 8) * U23 * ref["A_H"], (T + 2) * (V + 8) * U23 * ref["A_CE"]
    err_h, err_ce = np.abs(tot[:, 0] - ref["H"]), np.abs(tot[:, 1] - ref["CE"])
    frac = max((err_h / np.maximum(bound_h, 1e-300)).max(), (err_ce / np.maximum(bound_ce, 1e-300)).max())
    print("worst |total - ref| / bound:", frac, "H", ref["H"], "CE", ref["CE"])
    assert np.all(err_h <= bound_h) and np.all(err_ce <= bound_ce), frac
    kl = (totals[:, 1] - totals[:, 0]).astype(np.float64)                  # one fp32 subtraction, as the sampler forms it
    assert np.all(np.abs(kl - (ref["CE"] - ref["H"])) <= bound_h + bound_ce)
    if V == 1:
        assert np.all(totals == 0.0) and np.all(visits == 1.0) and np.all(open_mass == 0.0)
    else:
        assert np.all(ref["CE"] - ref["H"] > 0.0) and np.all(ref["H"] > 0.0)

    rel = (T + 1) * (V + 8) * U24
    ok = ref["visits"] >= 1e-30
    assert np.all(np.abs(visits.astype(np.float64)[ok] / ref["visits"][ok] - 1.0) <= rel)
    assert np.all(visits >= 0.0)
    ok = ref["open_mass"] >= 1e-30
    assert np.all(np.abs(open_mass.astype(np.float64)[ok] / ref["open_mass"][ok] - 1.0) <= rel)

    # visits against the marginals kernel's alive summed over the steps
    L = _lib()
    alive = torch.empty(B, T, V, dtype=torch.float32, device="cuda")
    L.call("arcvae_dec_chain_marginals", L.ptr(tp), L.ptr(lp), L.ptr(alive), B, V, T, end, float(temp), L.stream_ptr())
    summed = alive.double().sum(1).cpu().numpy()
    ok = summed >= 1e-30
    assert np.all(np.abs(visits.astype(np.float64)[ok] / summed[ok] - 1.0) <= rel)

    # bitwise repeatable
    again = _expect(tp, lp, cost, 2, B, V, T, end, temp)
    h2, c2 = _row_costs(tp, lp, temp, tq, lq, temp_q, B * V, V)
    for a, b in zip((totals, visits, open_mass, h.cpu().numpy(), c.cpu().numpy()), again + (h2.cpu().numpy(), c2.cpu().numpy())):
        np.testing.assert_array_equal(_bits(a), _bits(b))

    # Q = P (a second copy of the table: other pointers, the same values): c == h and CE == H, bit for bit
    hs, cs = _row_costs(tp, lp, temp, tp.clone(), lp.clone(), temp, B * V, V)
    np.testing.assert_array_equal(_bits(hs.cpu().numpy()), _bits(cs.cpu().numpy()))
    np.testing.assert_array_equal(_bits(hs.cpu().numpy()), _bits(h.cpu().numpy()))
    same, _, _ = _expect(tp, lp, torch.stack([hs, cs]).contiguous(), 2, B, V, T, end, temp)
    np.testing.assert_array_equal(_bits(same[:, 0]), _bits(same[:, 1]))
    np.testing.assert_array_equal(_bits(same[:, 0]), _bits(totals[:, 0]))
    # h alone (no q): the same bits, and c is not asked for
    h1, _ = _row_costs(tp, lp, temp, None, None, temp_q, B * V, V)
    np.testing.assert_array_equal(_bits(h1.cpu().numpy()), _bits(h.cpu().numpy()))

    # an output whose pointer is NULL is left untouched; the others keep their bits (one cost: the first total alone)
    t1, v1, o1 = _expect(tp, lp, cost, 1, B, V, T, end, temp, visits=False, open_mass=False)
    np.testing.assert_array_equal(_bits(t1[:, 0]), _bits(totals[:, 0]))
    assert np.all(v1 == -7.0) and np.all(o1 == -7.0)
    t2, v2, o2 = _expect(tp, lp, cost, 2, B, V, T, end, temp, totals=False, open_mass=False)
    np.testing.assert_array_equal(_bits(v2), _bits(visits))
    assert np.all(t2 == -7.0) and np.all(o2 == -7.0)
    t3, v3, o3 = _expect(tp, lp, cost, 2, B, V, T, end, temp, totals=False, visits=False)
    np.testing.assert_array_equal(_bits(o3), _bits(open_mass))
    assert np.all(t3 == -7.0) and np.all(v3 == -7.0)


def test_argument_errors_return_codes():
    L = _lib()
    lib = L.load()
    B, V, T, END = 2, 12, 8, 2
    table = torch.zeros(B * 257, 257, device="cuda")            # (large enough for the V = 257 call, should it launch)
    lse = torch.full((B * 257,), float(np.log(12.0)), device="cuda")
    h, c = torch.zeros(B * 257, device="cuda"), torch.zeros(B * 257, device="cuda")
    cost = torch.zeros(4, B * 257, device="cuda")
    totals, visits, open_mass = torch.zeros(B, 4, device="cuda"), torch.zeros(B, 257, device="cuda"), torch.zeros(B, device="cuda")

    def rc(V_=V, R_=None, tp=1.0, tq=1.0, xp=table, lp=lse, xq=table, lq=lse, h_=h, c_=c):
        return lib.arcvae_dec_row_costs(L.ptr(xp), L.ptr(lp), tp, L.ptr(xq), L.ptr(lq), tq, L.ptr(h_), L.ptr(c_),
                                        B * V_ if R_ is None else R_, V_, L.stream_ptr())

    def ex(V_=V, T_=T, end=END, temp=1.0, n=2, cost_=cost, totals_=totals, visits_=visits, open_=open_mass, xp=table, lp=lse):
        return lib.arcvae_dec_chain_expect(L.ptr(xp), L.ptr(lp), L.ptr(cost_), n, L.ptr(totals_), L.ptr(visits_), L.ptr(open_), B,
                                           V_, T_, end, temp, L.stream_ptr())

    assert rc(V_=0, R_=B) == -1 and rc(V_=257) == -1 and ex(V_=0) == -1 and ex(V_=257) == -1
    assert rc(R_=0) == -1
    assert ex(end=-1) == -1 and ex(end=V) == -1
    assert ex(T_=0) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rc(tp=bad) == -1 and rc(tq=bad) == -1 and ex(temp=bad) == -1
        assert rc(tq=bad, xq=None, lq=None, c_=None) == -1      # the second temperature is checked with or without q
    assert ex(n=-1) == -1 and ex(n=5) == -1
    assert ex(cost_=None) == -1 and ex(totals_=None) == -1
    assert ex(n=0) == -1 and ex(n=0, cost_=None) == -1 and ex(n=0, totals_=None) == -1      # (NULL iff n_cost == 0)
    assert rc(xq=None) == -1 and rc(lq=None) == -1 and rc(c_=None) == -1
    assert rc(xq=None, lq=None) == -1 and rc(xq=None, c_=None) == -1 and rc(lq=None, c_=None) == -1
    assert rc(xp=None) == -1 and rc(lp=None) == -1 and rc(h_=None) == -1 and ex(xp=None) == -1 and ex(lp=None) == -1
    assert ex(n=0, cost_=None, totals_=None, visits_=None, open_=None) == -1                 # no output asked for
    # and the valid calls still run
    assert rc() == 0 and rc(xq=None, lq=None, c_=None) == 0
    assert ex() == 0 and ex(n=0, cost_=None, totals_=None) == 0 and ex(visits_=None, open_=None) == 0
    assert ex(n=0, cost_=None, totals_=None, visits_=None) == 0
    torch.cuda.synchronize()
    # a table of zeros at lse = log V: every row uniform, h = log V
    assert np.all(np.abs(h.cpu().numpy()[:B * V] - np.log(12.0)) <= 1e-5)
    # ... and the expected length sum_t (11/12)^t (visits [B, V] at V 12 fills the head of the buffer)
    assert abs(visits.cpu().numpy().reshape(-1)[:B * V].sum() - B * 12 * (1 - (11 / 12) ** T)) <= 1e-3


# ---- model level: TINY, B 64 ---------------------------------------------------------------------------------------------------
B_M, T_M, END = 64, 12, 2


@pytest.fixture(scope="module")
def model():
    """The sampler, two sets of conditions and the fp64 reference on the decoder's OWN two tables (P: cond at temperature 1,
    Q: shifted conditions at temperature 1.4), built through the decoder's public path and computed once."""
    cfg, params, vae, cond, _ = ending_model(B_M, END)
    samp = vae.decoder_sampling
    dec = samp.decoder
    # (the weights are a random initialisation and the chain is nearly flat in the conditions: in fp64 a shift of s moves a row
    # by about 7.5e-6 s^2 nats at H = 34.3, whose fp32 rounding is about 1e-5 -- so the shift is large: measured on an MI355X, the smallest row's KL is 1.9e-3)
    cond_q = (cond + 32.0).astype(np.float32)
    temp_p, temp_q = 1.0, 1.4
    V = cfg.V
    ws, _ = dec.load_conditions(cond, T_M)
    dec.dense_table(ws)
    tab_p = ws.logits.clone()
    lse_p = dec.table_lse(ws, temp_p)
    lse_p_hot = dec.table_lse(ws, temp_q)
    ws, _ = dec.load_conditions(cond_q, T_M)
    dec.dense_table(ws)
    tab_q = ws.logits.clone()
    lse_q = dec.table_lse(ws, temp_q)
    torch.cuda.synchronize()
    tab_p, lse_p, lse_p_hot, tab_q, lse_q = (a.cpu().numpy() for a in (tab_p, lse_p, lse_p_hot, tab_q, lse_q))
    lp_p = R.step_terms(tab_p, lse_p, temp_p)
    ref = N.expectations(lp_p, R.step_terms(tab_q, lse_q, temp_q), B_M, V, T_M, END)
    ref_hot = N.expectations(lp_p, R.step_terms(tab_p, lse_p_hot, temp_q), B_M, V, T_M, END)
    return dict(cfg=cfg, vae=vae, samp=samp, cond=cond, cond_q=cond_q, temp_p=temp_p, temp_q=temp_q, ref=ref, ref_hot=ref_hot)


def test_methods_against_fp64(model):
    """Every method against the fp64 restatement on the decoder's own tables, inside the kernel bounds (the expected length adds
    one sum of V non-negative terms to visits' bound: (T + 1)(V + 8) u + V u <= (T + 2)(V + 8) u)."""
    samp, cond, cond_q, ref, V = model["samp"], model["cond"], model["cond_q"], model["ref"], model["cfg"].V
    bound_h, bound_ce = (T_M + 2) * (V + 8) * U23 * ref["A_H"], (T_M + 2) * (V + 8) * U23 * ref["A_CE"]
    H = samp.sequence_entropy(cond, max_length=T_M, temperature=model["temp_p"])
    assert H.shape == (B_M,) and H.dtype == torch.float32
    err = np.abs(H.cpu().numpy().astype(np.float64) - ref["H"])
    print("worst |H - ref| / bound:", (err / bound_h).max(), "H", ref["H"].min(), ref["H"].max())
    assert np.all(err <= bound_h)
    counts = samp.expected_token_counts(cond, max_length=T_M, temperature=model["temp_p"])
    assert counts.shape == (B_M, V) and counts.dtype == torch.float32
    ok = ref["visits"] >= 1e-30
    got = counts.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got[ok] / ref["visits"][ok] - 1.0) <= (T_M + 1) * (V + 8) * U24)
    length = samp.expected_length(cond, max_length=T_M, temperature=model["temp_p"])
    assert length.shape == (B_M,)
    rlen = ref["visits"].sum(axis=1)
    assert np.all(np.abs(length.cpu().numpy().astype(np.float64) / rlen - 1.0) <= (T_M + 2) * (V + 8) * U24)
    assert np.all(rlen > 1.0) and np.all(rlen < T_M)
    kl, ce, h = samp.sequence_divergence(cond, other_conditions=cond_q, other_temperature=model["temp_q"], max_length=T_M,
                                         temperature=model["temp_p"])
    for a in (kl, ce, h):
        assert a.shape == (B_M,) and a.dtype == torch.float32
    np.testing.assert_array_equal(_bits(h.cpu().numpy()), _bits(H.cpu().numpy()))
    assert np.all(np.abs(ce.cpu().numpy().astype(np.float64) - ref["CE"]) <= bound_ce)
    assert np.all(np.abs(kl.cpu().numpy().astype(np.float64) - (ref["CE"] - ref["H"])) <= bound_h + bound_ce)
    assert np.all(kl.cpu().numpy() > 0.0)                       # shifted conditions (and another temperature): every row moves
    # the temperature alone
    hot = model["ref_hot"]
    kl_t, ce_t, _ = samp.sequence_divergence(cond, other_temperature=model["temp_q"], max_length=T_M, temperature=model["temp_p"])
    assert np.all(np.abs(ce_t.cpu().numpy().astype(np.float64) - hot["CE"]) <= (T_M + 2) * (V + 8) * U23 * hot["A_CE"])
    assert np.all(kl_t.cpu().numpy() > 0.0)


def test_divergence_identities(model):
    samp, vae, cond, cond_q, cfg = model["samp"], model["vae"], model["cond"], model["cond_q"], model["cfg"]
    H = samp.sequence_entropy(cond, max_length=T_M).cpu().numpy()
    kl, ce, h = (a.cpu().numpy() for a in samp.sequence_divergence(cond, max_length=T_M))
    assert np.all(kl == 0.0)
    np.testing.assert_array_equal(_bits(ce), _bits(H))
    np.testing.assert_array_equal(_bits(h), _bits(H))
    kl_c, _, _ = samp.sequence_divergence(cond, other_conditions=cond_q, max_length=T_M)
    print("min kl against shifted conditions:", kl_c.min().item())
    assert np.all(kl_c.cpu().numpy() > 0.0)                     # against shifted conditions: every row
    np.testing.assert_array_equal(_bits(samp.sequence_entropy(cond, max_length=T_M).cpu().numpy()), _bits(H))   # (P's table held)
    # a second sampler loaded from the same decoder is the same distribution
    from models.decoder_sampling import MLXAutoregressiveDecoderSampling
    twin = MLXAutoregressiveDecoderSampling(cfg.V, cfg.E, cfg.H, cfg.Z, cfg.C, cfg.L, end_token=END,
                                            generator=torch.Generator().manual_seed(1))
    twin.load_from_decoder(vae.decoder)
    kl_o, ce_o, _ = samp.sequence_divergence(cond, other=twin, max_length=T_M)
    assert np.all(kl_o.cpu().numpy() == 0.0)
    np.testing.assert_array_equal(_bits(ce_o.cpu().numpy()), _bits(H))
    # the expected length is the length distribution's mean, an open outcome counting max_length
    ld = samp.length_distribution(cond, max_length=T_M).cpu().numpy().astype(np.float64)
    mean = ld @ np.concatenate([np.arange(1, T_M + 1), [T_M]]).astype(np.float64)
    length = samp.expected_length(cond, max_length=T_M).cpu().numpy().astype(np.float64)
    assert np.all(np.abs(length - mean) <= 1e-5 * T_M)
    counts = samp.expected_token_counts(cond, max_length=T_M).cpu().numpy()
    assert np.all((counts[:, END] > 0.0) & (counts[:, END] <= 1.0 + 1e-5))              # P(ended within max_length)


def test_value_errors(model):
    samp, cond, cfg = model["samp"], model["cond"], model["cfg"]
    from models.decoder_sampling import MLXAutoregressiveDecoderSampling
    for method in (samp.sequence_entropy, samp.expected_token_counts, samp.expected_length, samp.sequence_divergence):
        for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
                    dict(max_length=0)):
            with pytest.raises(ValueError):
                method(cond, **{"max_length": T_M, **bad})
    for bad in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            samp.sequence_divergence(cond, other_temperature=bad, max_length=T_M)
    with pytest.raises(ValueError):
        samp.sequence_divergence(cond, other_conditions=cond[:B_M - 1], max_length=T_M)      # mismatched B
    small = MLXAutoregressiveDecoderSampling(cfg.V - 1, cfg.E, cfg.H, cfg.Z, cfg.C, cfg.L, end_token=END,
                                             generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError):
        samp.sequence_divergence(cond, other=small, max_length=T_M)                          # mismatched vocabulary
    other_end = MLXAutoregressiveDecoderSampling(cfg.V, cfg.E, cfg.H, cfg.Z, cfg.C, cfg.L, end_token=3,
                                                 generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError):
        samp.sequence_divergence(cond, other=other_end, max_length=T_M)
    with pytest.raises(ValueError):
        samp.sequence_divergence(cond, other=samp.decoder, max_length=T_M)
