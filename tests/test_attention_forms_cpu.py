"""What tests/attention_forms.py can see, without a GPU: the rounding-point emulation of the correct statement stays within
MARGIN (and prints the maximum MARGIN was taken from), and every seeded defect -- a torch restatement of the kernels with one
thing wrong -- is rejected, by the third of dqkv it touches where it touches only one.  L in {33, 50, 97}, 5 heads, both masks.

Each defect's docstring records whether the tolerances of the direct tests that existed before this checker (forward
|err| <= 2e-2 + 2e-2 |ref| per element, test_gpu_kernels.py::test_attention; backward max |err| < 3e-2 absmax(dqkv) and cosine >
0.999, test_gpu_train.py::test_attention_backward) reject the same restatement: `old` below, printed per case."""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_forms as AF

H = 5
W = H * AF.HD
LS = (33, 50, 97)
CASES = [(L, causal) for L in LS for causal in (False, True)]


def setup(L, causal, regime, lay=AF.WINDOW, rows=None, seed=0):
    rows = rows or AF.Rows.fixed(L, 3)
    d = AF.make_data(rows, H, regime, 100 * L + causal + seed)
    b = AF.Buffers(d, rows, H, lay, "cpu", L)
    r = AF.reference(b.view(b.qkv), b.view(b.dout), H, causal, rows)
    return rows, b, r, AF.bound(r)


def store(prev, lay, values, front=0, nzero=0):
    """What a kernel that computed `values` (fp64 of bf16 values) for the block's rows, and zeroed nzero pad rows, leaves behind."""
    got = prev.clone()
    n, w = values.shape
    got[front + lay.base:front + lay.base + n, lay.col0:lay.col0 + w] = values.to(prev.dtype)
    got[front + lay.base + n:front + lay.base + n + nzero, lay.col0:lay.col0 + w] = 0
    return got


def judge(e, r, bd, b, rows, lay):
    """(worst of out, worst per third of dqkv) of the restatement e against the correct reference r."""
    exp, bnd, st = AF.expected(b.out0, lay, r.O_rows, bd.O_rows, rows.pad_rows)
    wo = AF.worst(store(b.out0, lay, e.O_rows, nzero=rows.pad_rows), exp, bnd, st, b.out0)
    if not hasattr(e, "dQ"):
        return wo, None
    cat = lambda x: torch.cat([x.dQ_rows, x.dK_rows, x.dV_rows], 1)
    exp, bnd, st = AF.expected(b.dqkv0, lay, cat(r), cat(bd), rows.pad_rows)
    return wo, AF.worst(store(b.dqkv0, lay, cat(e), nzero=rows.pad_rows), exp, bnd, st, b.dqkv0, AF.thirds(lay, H))


def old(e, r):
    """Do the earlier direct tests' tolerances reject e?  (forward, backward)"""
    fwd = bool(((e.O_rows - r.O_rows).abs() > 2e-2 + 2e-2 * r.O_rows.abs()).any())
    if not hasattr(e, "dQ"):
        return fwd, None
    cat = lambda x: torch.cat([x.dQ_rows, x.dK_rows, x.dV_rows], 1)
    g, ref = cat(e), cat(r)
    rel = float((g - ref).abs().max() / ref.abs().max())
    cos = float(F.cosine_similarity(g.flatten(), ref.flatten(), dim=0))
    return fwd, rel >= 3e-2 or cos <= 0.999


def edited(b, rows, causal, edit, **kw):
    return AF.emulate(AF.reference(b.view(b.qkv), b.view(b.dout), H, causal, rows, edit=edit), **kw)


def test_correct_emulation_is_within_margin():
    """Both layouts through whole poisoned buffers at L = 33 / 50 / 97, then the emulation over every case of the GPU sweep:
    the measured maxima are printed, and EMULATION_MAX (MARGIN / 2) is that maximum rounded up, no more."""
    mo = md = 0.0
    for L, causal in CASES:
        for regime in AF.REGIMES:
            for lay in AF.LAYOUTS:
                rows, b, r, bd = setup(L, causal, regime, lay)
                wo, wd = judge(AF.emulate(r), r, bd, b, rows, lay)
                assert AF.passes(wo, "fwd") and AF.passes(wd, "bwd"), (L, causal, regime, lay.name, wo, wd)
                mo, md = max(mo, float(wo)), max(md, float(wd.max()))
    for lens in AF.PACKED:
        rows = AF.Rows(lens, True, 9)
        rows, b, r, bd = setup(rows.L, True, "plain", AF.WINDOW, rows)
        wo, wd = judge(AF.emulate(r), r, bd, b, rows, AF.WINDOW)
        assert AF.passes(wo, "fwd") and AF.passes(wd, "bwd"), (lens, wo, wd)
        mo, md = max(mo, float(wo)), max(md, float(wd.max()))
    print(f"\nemulation: worst ratio forward {mo:.3f} (EMULATION_MAX {AF.EMULATION_MAX['fwd']}, MARGIN {AF.MARGIN['fwd']}), "
          f"backward {md:.3f} (EMULATION_MAX {AF.EMULATION_MAX['bwd']}, MARGIN {AF.MARGIN['bwd']:.2f})")
    assert AF.MARGIN == {k: 2 * v for k, v in AF.EMULATION_MAX.items()}
    top = AF.measure_emulation()                         # the whole sweep's cases: what EMULATION_MAX was taken from
    print(f"emulation over the GPU sweep's cases: {top}")
    for kind, m in (("fwd", max(top["fwd"], top["lastq"], mo)), ("bwd", max(top["bwd"], md))):
        assert 0.95 * AF.EMULATION_MAX[kind] <= m <= AF.EMULATION_MAX[kind], (kind, m)


@pytest.mark.parametrize("L,causal", CASES)
def test_single_query_emulation_and_one_key_short(L, causal):
    """Single-query forms: the emulation passes; taking last_row[b] - row0 keys (one short) is rejected.
    old: the forward tolerance rejects it in 5 of the 6 cases (the dropped key is the query's own position, which usually carries
    weight); L = 97 with key counts 94, 2, 97 passes it at a ratio of 9 here."""
    rows = AF.Rows.fixed(L, 3)
    nk = [L - 3, 2, L] if causal else [L] * 3
    for lay in AF.LAYOUTS:
        d = AF.make_data(rows, H, "plain", L, nq=3)
        b = AF.Buffers(d, rows, H, lay, "cpu", L, front=7, single=True)
        ref = lambda nkeys: AF.reference(b.view(b.qkv), None, H, False, rows, q=b.view(b.qc), nkeys=nkeys, row0=7)
        r = ref(nk)
        exp, bnd, st = AF.expected(b.out0, lay, r.O_rows, AF.bound(r).O_rows)
        assert AF.passes(AF.worst(store(b.out0, lay, AF.emulate(r).O_rows), exp, bnd, st, b.out0), "fwd")
        short = AF.emulate(ref([n - 1 for n in nk]))
        w = AF.worst(store(b.out0, lay, short.O_rows), exp, bnd, st, b.out0)
        print(f"\none key short L={L}: worst {float(w):.3g}, old {old(short, r)[0]}")
        assert float(w) > AF.MARGIN["fwd"]


@pytest.mark.parametrize("L,causal", CASES)
def test_delta_from_the_stored_output_is_rejected(L, causal):
    """delta = sum_d dO O from the bf16 O (the defect csrc/attention_bwd.hip describes) moves dQ and dK, not dV: the dq and dk
    thirds reject it (ratios 13 - 270), the dv third and the forward pass.
    old: NOT rejected in the plain, sharp and wide regimes (all 18 cases); in the offset regime (v + 3 makes O, and with it O's
    rounding error, four times larger) 4 of the 6 cases exceed the 3 % -- a regime no earlier test ran."""
    for regime in AF.REGIMES:
        rows, b, r, bd = setup(L, causal, regime)
        e = AF.emulate(r, delta_from_o=True)
        wo, wd = judge(e, r, bd, b, rows, AF.WINDOW)
        print(f"\ndelta from o L={L} causal={causal} {regime}: thirds {[round(float(x), 1) for x in wd]}, old {old(e, r)}")
        assert AF.passes(wo, "fwd") and AF.passes(wd[2], "bwd")
        assert float(wd[0]) > AF.MARGIN["bwd"] and float(wd[1]) > AF.MARGIN["bwd"]


def drop_last_key(p):
    lens = torch.tensor(p.rows.lens)
    pos = torch.arange(p.kvalid.shape[1])
    last = (pos[None, :] == lens[:, None] - 1) & (lens[:, None] % 32 != 0)
    p.mask = p.mask & ~last[:, None, None, :]


@pytest.mark.parametrize("regime", ["plain", "sharp"])
@pytest.mark.parametrize("L,causal", CASES)
def test_dropped_last_key_of_a_ragged_tile_is_rejected(L, causal, regime):
    """The last key of a ragged 32-key tile masked away.  Under the causal mask only the last query sees it: one row of O and dQ,
    but every element of that key's dK and dV rows (their reference is nonzero, the restatement stores 0): the dk and dv thirds
    reject it in both regimes, whatever the forward does.
    old: rejected without the causal mask.  With it: plain, L = 33 passes the backward tolerance (the forward one catches the
    one query row); sharp, L = 33 and 50 pass BOTH (forward ratio here 0.9: the last query gives its own key no weight, so only
    the key's dK / dV rows, small against absmax(dqkv), are wrong); L = 97 is rejected."""
    rows, b, r, bd = setup(L, causal, regime)
    e = edited(b, rows, causal, drop_last_key)
    wo, wd = judge(e, r, bd, b, rows, AF.WINDOW)
    print(f"\ndropped key L={L} causal={causal} {regime}: out {float(wo):.3g} thirds {[round(float(x), 1) for x in wd]}, old {old(e, r)}")
    assert float(wd[1]) > AF.MARGIN["bwd"] and float(wd[2]) > AF.MARGIN["bwd"]
    if regime == "plain":                              # (sharp + causal: the one query that sees the key may give it no weight)
        assert float(wo) > AF.MARGIN["fwd"]


@pytest.mark.parametrize("L", LS)
def test_causal_mask_one_position_too_wide_is_rejected(L):
    """Key q + 1 visible to query q.  old: rejected (every row but the last changes)."""
    def wide(p):
        pos = torch.arange(p.kvalid.shape[1])
        p.mask = p.kvalid[:, None, None, :] & (pos[None, :] <= pos[:, None] + 1)
    rows, b, r, bd = setup(L, True, "plain")
    e = edited(b, rows, True, wide)
    wo, wd = judge(e, r, bd, b, rows, AF.WINDOW)
    print(f"\nwide mask L={L}: out {float(wo):.3g} thirds {[round(float(x), 1) for x in wd]}, old {old(e, r)}")
    assert float(wo) > AF.MARGIN["fwd"] and bool((wd > AF.MARGIN["bwd"]).all())


@pytest.mark.parametrize("L,causal", CASES)
def test_wrong_head_and_wrong_head_count_are_rejected(L, causal):
    """Head h reading head h + 1's V; the column offsets of k and v computed with 12 heads where heads is 5 (the reads then
    land in other columns and rows of the same buffer).  old: both rejected (uncorrelated values everywhere)."""
    rows, b, r, bd = setup(L, causal, "plain", AF.TIGHT)

    def next_head(p):
        p.V = torch.roll(p.V, -1, 1)
    e = edited(b, rows, causal, next_head)
    wo, wd = judge(e, r, bd, b, rows, AF.TIGHT)
    assert float(wo) > AF.MARGIN["fwd"] and float(wd[0]) > AF.MARGIN["bwd"] and float(wd[1]) > AF.MARGIN["bwd"]
    assert AF.passes(wd[2], "bwd")                     # dV = P^T dO does not read V: only a per-third ratio says so
    flat = torch.nan_to_num(b.qkv, 0.5).flatten()                        # (finite: this restatement is about the values)
    at = torch.arange(rows.live)[:, None] * b.ldq + torch.arange(W)[None, :]
    wrong = torch.cat([b.qkv[:rows.live, :W], flat[(at + 12 * AF.HD) % flat.numel()], flat[(at + 24 * AF.HD) % flat.numel()]], 1)
    e2 = AF.emulate(AF.reference(wrong, b.view(b.dout), H, causal, rows))
    wo2, wd2 = judge(e2, r, bd, b, rows, AF.TIGHT)
    print(f"\nnext head's V L={L}: {float(wo):.3g} {wd.tolist()} old {old(e, r)}; 12-head offsets: {float(wo2):.3g} {wd2.tolist()} old {old(e2, r)}")
    assert float(wo2) > AF.MARGIN["fwd"] and bool((wd2 > AF.MARGIN["bwd"]).all())


@pytest.mark.parametrize("L,causal", CASES)
def test_k_offset_leaking_into_p_is_rejected(L, causal):
    """offset regime (k + 2 shifts every score of a query by 2 sum_c q): the row maximum and sum taken from the scores WITHOUT
    the offset, the exponentials with it, so P carries exp(2 sum_c q) per query.  old: rejected."""
    rows, b, r, bd = setup(L, causal, "offset")
    e = AF.emulate(r, norm_k_shift=AF.K_OFFSET)
    wo, wd = judge(e, r, bd, b, rows, AF.WINDOW)
    print(f"\nk offset in P L={L} causal={causal}: out {float(wo):.3g} thirds {[round(float(x), 1) for x in wd]}, old {old(e, r)}")
    assert float(wo) > AF.MARGIN["fwd"] and bool((wd > AF.MARGIN["bwd"]).all())


@pytest.mark.parametrize("lens", AF.PACKED, ids=lambda l: "-".join(map(str, l)))
def test_pad_rows_left_alone_are_rejected(lens):
    """Packed forms: the pad rows behind cu[nsamples] must be exactly zero (bound 0); a restatement that leaves them is inf.
    old: rejected where the test looks at the pad rows (test_gpu_pack.py does)."""
    rows = AF.Rows(lens, True, 6)
    rows, b, r, bd = setup(rows.L, True, "plain", AF.WINDOW, rows)
    e = AF.emulate(r)
    cat = lambda x: torch.cat([x.dQ_rows, x.dK_rows, x.dV_rows], 1)
    for prev, val, ref_, bnd_, kind in ((b.out0, e.O_rows, r.O_rows, bd.O_rows, "fwd"), (b.dqkv0, cat(e), cat(r), cat(bd), "bwd")):
        exp, bnd, st = AF.expected(prev, AF.WINDOW, ref_, bnd_, rows.pad_rows)
        got = store(prev, AF.WINDOW, val)
        assert float(AF.worst(got, exp, bnd, st, prev)) == math.inf
        got[AF.WINDOW.base + rows.live:AF.WINDOW.base + rows.block, AF.WINDOW.col0:AF.WINDOW.col0 + val.shape[1]] = 0
        assert AF.passes(AF.worst(got, exp, bnd, st, prev), kind)
        got[AF.WINDOW.base + rows.block, AF.WINDOW.col0] = 0              # ... and one row further is a write outside the contract
        assert float(AF.worst(got, exp, bnd, st, prev)) == math.inf


@pytest.mark.parametrize("L,causal", CASES)
def test_mask_by_multiplication_gives_nan_and_a_stray_write_inf(L, causal):
    """The padded keys of the last 32-key tile read from the rows behind the sample and `masked` by P = 0: 0 * NaN.  The rows
    behind the last sample are NaN in attention_forms.Buffers, so its outputs are NaN and worst() is nan; on randn rows (what the
    earlier tests put there) the same restatement is exact.  A write one row past the last live row is inf.
    old: not seen (finite rows behind the block; the stray write only where a test checks the rows behind)."""
    rows, b, r, bd = setup(L, causal, "plain")
    LP = (L + 31) // 32 * 32
    view, pos = b.view(b.qkv), torch.arange(LP)
    idx = torch.tensor(rows.starts)[:, None] + pos[None, :]
    idx = idx.clamp(max=view.shape[0] - 1)                              # (the buffer's last row stands for every row behind it)
    g = lambda col: view[idx.reshape(-1), col:col + W].double().view(3, LP, H, AF.HD).permute(0, 2, 1, 3)
    K, V = torch.nan_to_num(g(W), 0.0), g(2 * W)                        # K through a select (as the kernels do), V through 0 * V
    Q = r.p.Q
    mask = (pos[None, :] < L) & ((pos[None, :] <= torch.arange(L)[:, None]) if causal else torch.ones(L, LP, dtype=torch.bool))
    P = torch.softmax((Q @ K.transpose(-1, -2)).masked_fill(~mask, -math.inf), -1)
    O = (P[..., None] * V[:, :, None, :, :]).sum(-2)
    o_rows = AF.bf16_round(O.permute(0, 2, 1, 3).reshape(3 * L, W))
    exp, bnd, st = AF.expected(b.out0, AF.WINDOW, r.O_rows, bd.O_rows)
    w = AF.worst(store(b.out0, AF.WINDOW, o_rows), exp, bnd, st, b.out0)
    assert math.isnan(float(w))
    assert bool(o_rows[:2 * L].isfinite().all())                        # samples 0 and 1 multiply finite rows (the next sample's)
    good = store(b.out0, AF.WINDOW, AF.emulate(r).O_rows)
    assert AF.passes(AF.worst(good, exp, bnd, st, b.out0), "fwd")
    good[AF.WINDOW.base + rows.live, AF.WINDOW.col0 + 8] = 1.0
    assert float(AF.worst(good, exp, bnd, st, b.out0)) == math.inf
