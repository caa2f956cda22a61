"""tests/gemm_forms.py reports what it is there to report (no GPU needed).

The stand-in for a correct kernel is written here a second time, independently of gemm_forms.reference: fp32 accumulation
(torch's fp32 matmul of the bf16-valued operands), the epilogue in fp32 in the header's order, one rounding to the output type.
Undamaged it must pass gemm_forms.bounds on every form any kernel is promised to take, at the GPU sweep's dense shape and data
(M = 300, N = 264 / 266, K = 128; x ~ N(0, 1), w ~ N(0, 0.1), bias and residual ~ N(0, 1)).  Then one defect at a time -- the ways
an epilogue branch goes wrong -- is planted into it and must be reported on EVERY promised form on which it changes the
arithmetic at all.  That is what lets the GPU sweep reuse the suite's loose bf16 bounds: each of these defects is O(1)."""
import os

import pytest
import torch

import gemm_forms as GF

M, G = 300, 49
N_VALUES = (264, 266)


@pytest.fixture(scope="module")
def problem():
    x, w, bias, acc = GF.dense_problem(M, max(N_VALUES), "cpu")
    acc32 = x[:M].float() @ w.float().t()
    rows = GF.buffer_rows(M, G)
    bufs = {(N, pad): GF.Buffers(rows, N + pad, "cpu", seed=100 + 16 * N + pad) for N in N_VALUES for pad in GF.LD_PADS}
    fs = [f for f in GF.forms(N_VALUES) if GF.promised(GF.GENERAL, f)]
    refs = {}
    for f in fs:
        b = bufs[(f.N, f.ld_pad)]
        refs[f] = GF.expected_of(acc, bias, f, G, b, b.prev32 if f.out_f32 else b.prev16)
    return acc32, bias, bufs, fs, refs


def emulate(acc32, bias, f, b, defect=None):
    """The whole output buffer a kernel with `defect` leaves behind for form f."""
    rpg, radd, roff = GF.scatter_of(f, G)
    N = f.N
    out, _ = b.out(f.out_f32)
    r = b.resid(f.resid_kind)
    rk, act = f.resid_kind, f.act
    m = torch.arange(M)
    grp = m // rpg
    srow = m + (grp + (1 if defect == "store row off by one group" else 0)) * radd + roff
    v = acc32[:, :N] * f.alpha
    if f.bias and defect != "bias dropped":
        v = v + bias[:N]
    if defect == "alpha applied to the bias as well" and f.bias:
        v = (acc32[:, :N] + bias[:N]) * f.alpha
    gelu = lambda t: t * torch.sigmoid(1.702 * t)
    late_gelu = defect == "QuickGELU after the residual"
    early_relu = defect == "ReLU before the residual"
    if act == 1 and not late_gelu:
        v = gelu(v)
    if act == 2 and early_relu:
        v = torch.relu(v)
    trow = m - grp * rpg + roff + (1 if defect == "table row off by one" else 0)
    if rk in (1, 2):
        rows = trow if (rk == 2 and defect == "bf16 residual read as the table row") else m
        v = v + r[rows, :N].float()
    elif rk == 3:
        rows = m if defect == "table residual read at row m" else trow
        v = v + r[rows, :N].float()
    if act == 1 and late_gelu:
        v = gelu(v)
    if act == 2 and not early_relu:
        v = torch.relu(v)
    at = m if defect == "kinds 5 / 6 read at the launch row" else srow
    if rk == 5:
        v = torch.where(r[at, :N].float() > 0, v, torch.zeros_like(v))
    elif rk == 6:
        v = v + r[at, :N].float()
    ncols = N - N % 4 if defect == "last N % 4 columns skipped" else N
    nrows = M - M % 32 if defect == "last M % 32 rows skipped" else M
    out[srow[:nrows], :ncols] = v[:nrows, :ncols].to(out.dtype)
    if defect == "one pad column overwritten":
        out[srow[7], N] = 0.0
    return out


# defect -> the forms on which it changes what the kernel computes
DEFECTS = {
    "bias dropped": lambda f: f.bias,
    "alpha applied to the bias as well": lambda f: f.bias and f.alpha != 1.0,
    "QuickGELU after the residual": lambda f: f.act == 1 and f.resid_kind in (1, 2, 3),
    "ReLU before the residual": lambda f: f.act == 2 and f.resid_kind in (1, 2, 3),
    "bf16 residual read as the table row": lambda f: f.resid_kind == 2 and f.scatter,     # (identity rows: row m is table row m)
    "table residual read at row m": lambda f: f.resid_kind == 3 and f.scatter,
    "table row off by one": lambda f: f.resid_kind == 3,
    "store row off by one group": lambda f: f.scatter,
    "kinds 5 / 6 read at the launch row": lambda f: f.resid_kind in (5, 6) and f.scatter,
    "last N % 4 columns skipped": lambda f: f.N % 4 != 0,
    "last M % 32 rows skipped": lambda f: True,
    "one pad column overwritten": lambda f: f.ld_pad > 0,
}


def _worst(problem, f, defect=None):
    acc32, bias, bufs, _, refs = problem
    b = bufs[(f.N, f.ld_pad)]
    got = emulate(acc32, bias, f, b, defect)
    expected, stored = refs[f]
    return float(GF.worst(got, expected, stored, b.prev32 if f.out_f32 else b.prev16, f.resid_kind))


def test_promise_table_is_not_empty_anywhere():
    """Every kernel is promised a good share of the product, and the general kernel's promise contains the others'."""
    all_forms = list(GF.forms(N_VALUES))
    assert len(all_forms) == 2 * 3 * 2 * 2 * 3 * 6 * 2 * 2
    general = {f for f in all_forms if GF.promised(GF.GENERAL, f)}
    for kernel in ("pp", "ppconv", "dense128", "dense192", "conv128", "conv192", "stream", "stream_conv", "f8"):
        mine = {f for f in all_forms if GF.promised(kernel, f)}
        assert len(mine) >= 432 and mine <= general, kernel       # 432: bias x alpha x act x kinds 0 - 2 x out x N x ld


def test_correct_emulation_passes_every_promised_form(problem):
    fs = problem[3]
    ratios = [_worst(problem, f) for f in fs]
    print(f"{len(fs)} forms, worst err / tol {max(ratios):.3g}")
    assert max(ratios) <= 1.0


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_is_reported(problem, defect):
    fs = [f for f in problem[3] if DEFECTS[defect](f)]
    assert len(fs) >= 16, "the defect must apply to a real share of the product"
    escaped = [f for f in fs if _worst(problem, f, defect) <= 1.0]
    assert not escaped, f"{defect}: escaped on {len(escaped)} of {len(fs)} forms, first {escaped[0]}"


def test_reference_passes_previous_contents_through(problem):
    """The expected buffer is the previous one outside the stored rows and columns, and the mask says exactly which those are."""
    _, _, bufs, fs, refs = problem
    f = next(f for f in fs if f.scatter and f.ld_pad and not f.out_f32 and f.N % 4)
    expected, stored = refs[f]
    prev = bufs[(f.N, f.ld_pad)].prev16
    assert int(stored.sum()) == M * f.N and not stored[:, f.N:].any() and not stored[0].any() and not stored[-2:].any()
    assert stored[49, :f.N].all() and not stored[50].any() and stored[51, :f.N].all()          # rows 48 -> 49, 49 -> 49 + 1 + 1 = 51
    assert torch.equal(expected[~stored], prev.double()[~stored])


def test_library_rejects_the_descriptor_holes():
    """msclip_gemm_variant is host code: resid_kind without a pointer, act out of range, ldo < N and a zero-sized conv output are
    "invalid" for every tile request (and do not crash the query)."""
    from msclip_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    labels = []
    for label, d in GF.rejected_descriptors():
        labels.append(label)
        assert hip.gemm_variant(d) == "invalid", label
    assert len(labels) >= 30
    ok = hip.describe_gemm(0, 300, 264, 128, resid_kind=1)
    assert hip.gemm_variant(ok) == "dense128"                                  # the same descriptor with its pointer is taken
    ok.resid_kind, ok.act, ok.out_kind = 6, 2, 0
    assert hip.gemm_variant(ok) == "invalid"                                   # accumulate is not combined with ReLU
    ok.act = 1
    assert hip.gemm_variant(ok) == "dense128"


# kernel -> (mode, tile, M, K, ldx, N values, scatter group, wg_cap values, conv geometry): the GPU sweep's cases, shapes only
ASKED = {
    "dense128": (0, 1, 300, 128, 128, (264, 266), 49, (0, 1), None),
    "dense192": (0, 6, 300, 128, 128, (264, 266), 49, (0, 1), None),
    "pp": (0, 4, 300, 128, 128, (264, 266), 49, (0, 1), None),
    "stream": (0, 5, 4099, 128, 96, (96, 40, 42), 49, (0,), None),
    "conv128": (1, 1, 392, 576, 0, (96, 98), 196, (0, 1), (14, 14, 64, 14, 14, 1, 1)),
    "conv192": (1, 6, 392, 576, 0, (96, 98), 196, (0, 1), (14, 14, 64, 14, 14, 1, 1)),
    "ppconv": (1, 4, 392, 576, 0, (96, 98), 196, (0, 1), (14, 14, 64, 14, 14, 1, 1)),
    "stream_conv": (1, 5, 9408, 448, 0, (96, 94), 3136, (0,), (112, 112, 48, 56, 56, 2, 1)),
}


@pytest.mark.parametrize("kernel", list(ASKED))
def test_library_answers_are_the_documented_ones(kernel):
    """msclip_gemm_variant on shape-only descriptors (dummy non-null pointers, no GPU work) for every form of every case of the
    GPU sweep: the asked-for kernel where the form is promised, "invalid" or the documented fall-back kernel where it is not --
    and the number of handed-on forms is the expected one, so that a new silent fall-back fails here."""
    from msclip_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    mode, tile, M_, K, ldx, n_values, g, wg_caps, geo = ASKED[kernel]

    class Dummy:
        ld = 0

        def data_ptr(self):
            return 4096

        def resid(self, kind):
            return self if kind else None

    own, elsewhere, wrong = GF.VARIANT.get(kernel, kernel), 0, []
    for f in GF.forms(n_values, wg_caps):
        d = hip.describe_gemm(mode, M_, f.N, K, tile=tile, conv=geo, ldx=ldx or None)
        b = Dummy()
        b.ld = f.N + f.ld_pad
        GF.fill_epilogue(d, f, g, b, b, b)
        name = hip.gemm_variant(d)
        if name != GF.expected_variant(kernel, f):
            wrong.append((f, name))
        elsewhere += name not in ("invalid", own)
    assert not wrong, f"{len(wrong)} forms, first {wrong[:3]}"
    assert elsewhere == GF.ELSEWHERE.get(kernel, 0)
