"""The epilogue contract of msclip_gemm / msclip_gemm_f8 (include/msclip_hip.h, the comment above msclip_gemm_desc) as a checker:

    v = alpha * acc + bias[n];  act 1: QuickGELU;  + resid (1: fp32 [m][n], 2: bf16 [m][n], 3: fp32 table row m % rpg + roff);
    act 2: ReLU;  resid_kind 5: keep v where resid[store row][n] > 0 / 6: + resid[store row][n] (bf16);
    store to row m + (m / rpg) * radd + roff, columns [0, N), as bf16 or fp32 -- and nothing else.

reference() states it in fp64 over a whole output BUFFER (pad columns, the gap rows of a scatter, rows past M), promised() says
which of the nine kernels behind the entry point the documentation lets take which form, bounds() are the suite's tolerances.
tests/test_gemm_forms_cpu.py shows that the checker reports every defect an epilogue branch can have at those tolerances;
tests/test_gpu_gemm_forms.py runs every kernel over the product of the forms.  No fixtures, no hooks: an ordinary module."""
import ctypes
import itertools
from collections import namedtuple

import torch

INT_MAX = 2 ** 31 - 1
BF = torch.bfloat16
K_DENSE = 128

# One epilogue form.  out_f32: fp32 (else bf16) output; scatter: rows stored to m + m / g + 1 (rpg = g, radd = roff = 1) instead
# of m; ld_pad: ldo = ldr = N + ld_pad; wg_cap: msclip_gemm_desc.wg_cap.
Form = namedtuple("Form", "bias alpha act resid_kind out_f32 scatter N ld_pad wg_cap")

RESID_KINDS = (0, 1, 2, 3, 5, 6)
# tight, padded by 8, and padded by 2: with N % 4 == 2 the last one gives leading dimensions that are multiples of 4 under a
# ragged N -- the only way to the element-wise tail path for resid_kind 5 / 6, which need ldr % 4 == 0
LD_PADS = (0, 8, 2)


def forms(n_values, wg_caps=(0,), resid_kinds=RESID_KINDS):
    """The full product of the axes, act x resid_kind x out kind x rows innermost."""
    for N, ld_pad, wg, bias, alpha, act, rk, f32, scatter in itertools.product(
            n_values, LD_PADS, wg_caps, (False, True), (1.0, 0.5), (0, 1, 2), resid_kinds, (False, True), (False, True)):
        yield Form(bias, alpha, act, rk, f32, scatter, N, ld_pad, wg)


# ---- what the documentation promises ---------------------------------------------------------------------------------------
# kernel names: msclip_gemm_variant's, plus "stream_conv" (the streaming kernel in implicit-conv mode: the same variant name
# "stream", but mode 1 admits resid_kind 5) and "f8" (msclip_gemm_f8: the dense ping-pong kernel on e4m3 operands).
CONV_KERNELS = ("conv128", "conv192", "ppconv", "stream_conv")
GENERAL = "conv128"            # the kernel whose promise contains every other kernel's: what the CPU checker test sweeps


def promised(kernel, f):
    """Does the documentation let `kernel` take form `f`?  Written from include/msclip_hip.h and the comments of
    csrc/gemm.hip::pick_variant / csrc/gemm_small.hip::msclip_gemm_small_eligible, not from running the library.

    Readings where the text was silent (each now stated in the header's comment):
      * resid_kind 5 / 6 need ldr % 4 == 0 although the element-wise tail path exists for them: pick_variant's comment-free
        `ldr & 3` test was the only statement; taken as the rule (the saved activation / the map accumulated into are bf16
        maps the engine always allocates 8-aligned).
      * resid_kind 6 with act 2: the header did not say on which side of the ReLU the accumulate sits, the contract line puts
        ReLU first, every kernel adds first.  Nothing launches the pair, so it is rejected rather than given a meaning.
      * msclip_gemm_f8 "same ... residual ... kinds": kinds 0 - 2 without a row scatter (its own argument check; the table
        residual and the scatter live in the guarded edge epilogue only, which the fp8 entry does not promise).
      * tile 5 / tile 4 on a form the streaming / implicit-conv ping-pong kernel does not carry is not an error: the library
        names the kernel that takes the launch instead ("dense128", "conv128").  promised() is about the kernel asked for,
        so such a form is not promised for it, and the sweep launches only what the asked-for kernel takes.
      * tile 6 in mode 1 takes any N ("N % 192 == 0" describes what auto picks)."""
    rk = f.resid_kind
    if rk == 5 and kernel not in CONV_KERNELS:                    # "resid_kind 5 (mode 1, ...)"
        return False
    if rk == 6 and f.out_f32:                                     # "resid_kind 6 (bf16 out, ...)"
        return False
    if rk in (5, 6) and (f.N + f.ld_pad) % 4:                     # ldr % 4 == 0
        return False
    if rk == 6 and f.act == 2:
        return False
    if rk in (5, 6) and kernel in ("pp", "ppconv", "f8"):         # "generic / streaming kernels": not tile 4
        return False
    if kernel in ("ppconv", "f8") and (rk == 3 or f.scatter):     # pick_variant: "rpg == INT_MAX && resid_kind != 3" for ppconv
        return False
    if kernel in ("stream", "stream_conv"):                       # msclip_gemm_small_eligible: "(row scatter: plain stores or the
        if rk == 3 or (f.scatter and rk in (1, 2)):               #  ReLU mask)", no table residual
            return False
    return True


VARIANT = {"stream_conv": "stream"}                               # kernel name here -> msclip_gemm_variant's name, where they differ


def expected_variant(kernel, f):
    """What msclip_gemm_variant must answer when `kernel` is asked for form f: its own name where the form is promised; where it
    is not, "invalid" -- or, on the two documented fall-back routes (include/msclip_hip.h: tile 5 -> the 128 x 128 kernels for a
    table residual and for a row scatter with a residual of kind 1 / 2; tile 4 in mode 1 -> "conv128" for a table residual and a
    row scatter), the kernel that takes the launch instead, provided that kernel is promised the form.  resid_kind 5 / 6 under
    tile 4 are refused outright, not handed on.  Any other answer is a silent fall-back nobody documented."""
    if promised(kernel, f):
        return VARIANT.get(kernel, kernel)
    other = {"stream": "dense128", "stream_conv": "conv128", "ppconv": "conv128"}.get(kernel)
    if other is None or (kernel == "ppconv" and f.resid_kind in (5, 6)) or not promised(other, f):
        return "invalid"
    return other


# forms of the sweep's cases (tests/test_gpu_gemm_forms.py) that the asked-for kernel hands to a 128 x 128 kernel on those routes;
# no other kernel hands any on
ELSEWHERE = {"stream": 864, "ppconv": 1440, "stream_conv": 576}


def small_m_takes(f):
    """Does the small-M kernel behind "dense128" carry form f (csrc/gemm_skinny.hip, the comment above skinny_eligible: no row
    scatter, no table / bf16 / masked residual, no ReLU, no workgroup cap)?  msclip_gemm_variant says "dense128" either way and
    the library has no query for which of the two kernels ran; this restates the documented conditions so that the sweep can at
    least say which of its forms were the small-M kernel's to take."""
    return f.resid_kind in (0, 1) and f.act in (0, 1) and not f.scatter and f.wg_cap == 0


# ---- the contract -----------------------------------------------------------------------------------------------------------
def bounds(out_dtype, resid_kind):
    """(atol, rtol) on |got - ref| against the unrounded fp64 reference: the suite's own (tests/test_gpu_kernels.py,
    tests/test_gpu_small_m.py): bf16 out 2e-2 + 1e-2 |ref|, with a bf16 residual or accumulate 3e-2 + 1e-2 |ref|, fp32 out
    2e-3 + 1e-4 |ref|."""
    if out_dtype == torch.float32:
        return 2e-3, 1e-4
    return (3e-2 if resid_kind in (2, 6) else 2e-2), 1e-2


def store_rows(M, rpg, radd, roff, device):
    m = torch.arange(M, device=device)
    return m + (m // rpg) * radd + roff


def reference(acc, *, bias, alpha, act, resid_kind, resid, rpg, radd, roff, prev):
    """-> (expected, stored): the whole output buffer the contract leaves behind, fp64 [rows, ldo], and the mask of the elements
    it stores.  acc: fp64 [M, N] contraction result (exact products of the bf16 / e4m3 operand values); bias: [N] or None;
    resid: the residual buffer as the kernel reads it, [rows, ldr] in the dtype of its kind (1, 3: fp32; 2, 5, 6: bf16);
    prev: what the output buffer held, [rows, ldo] in the output dtype -- it passes through wherever nothing is stored.
    The stored values are NOT rounded to the output type: bounds() were set against unrounded references."""
    M, N = acc.shape
    m = torch.arange(M, device=acc.device)
    grp = m // rpg
    srow = m + grp * radd + roff
    v = alpha * acc
    if bias is not None:
        v = v + bias.double()
    if act == 1:
        v = v * torch.sigmoid(1.702 * v)
    if resid_kind in (1, 2):
        v = v + resid[:M, :N].double()
    elif resid_kind == 3:
        v = v + resid[m - grp * rpg + roff, :N].double()
    if act == 2:
        v = torch.relu(v)
    if resid_kind == 5:
        v = torch.where(resid[srow, :N].double() > 0, v, torch.zeros_like(v))
    elif resid_kind == 6:
        v = v + resid[srow, :N].double()
    expected = prev.double().clone()
    expected[srow, :N] = v
    stored = torch.zeros(prev.shape, dtype=torch.bool, device=prev.device)
    stored[srow, :N] = True
    return expected, stored


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def worst(got, expected, stored, prev, resid_kind):
    """Worst |got - expected| / tolerance over the stored elements as a 0-dim tensor; inf if an element the contract does not
    store changed a bit, nan if a stored element is nan.  Passing means <= 1."""
    atol, rtol = bounds(got.dtype, resid_kind)
    ratio = (got.double() - expected).abs() / (atol + rtol * expected.abs())
    moved = _bits(got) != _bits(prev)
    inf = torch.full_like(ratio, float("inf"))
    return torch.where(stored, ratio, torch.where(moved, inf, torch.zeros_like(ratio))).max()


# ---- data -------------------------------------------------------------------------------------------------------------------
def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32, dev="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def as_rows(raw, rows, ld):
    return raw[:rows * ld].view(rows, ld)


class Buffers:
    """Output and residual buffers of one (rows, ld): every one holds rows * ld * 4 bytes whatever type it is read as, so that a
    form routed to the wrong branch computes a wrong number, never an address outside the buffer.  out16 / out32: the output
    (restored from prev16 / prev32 before every launch); r16 / r32: residual data N(0, 1) (r32 is also the table)."""

    def __init__(self, rows, ld, dev, seed):
        self.rows, self.ld = rows, ld
        self.raw_prev16 = rnd(2 * rows * ld, seed=seed, scale=4.0, dtype=BF, dev=dev)
        self.raw_prev32 = rnd(rows * ld, seed=seed + 1, scale=4.0, dev=dev)
        self.raw_out16, self.raw_out32 = self.raw_prev16.clone(), self.raw_prev32.clone()
        self.raw_r16 = rnd(2 * rows * ld, seed=seed + 2, dtype=BF, dev=dev)
        self.raw_r32 = rnd(rows * ld, seed=seed + 3, dev=dev)
        self.prev16, self.prev32 = as_rows(self.raw_prev16, rows, ld), as_rows(self.raw_prev32, rows, ld)
        self.out16, self.out32 = as_rows(self.raw_out16, rows, ld), as_rows(self.raw_out32, rows, ld)
        self.r16, self.r32 = as_rows(self.raw_r16, rows, ld), as_rows(self.raw_r32, rows, ld)

    def out(self, f32):
        """-> (out view, prev view) after restoring the output buffer."""
        if f32:
            self.raw_out32.copy_(self.raw_prev32)
            return self.out32, self.prev32
        self.raw_out16.copy_(self.raw_prev16)
        return self.out16, self.prev16

    def slack_moved(self):
        """Did the half of the bf16 output's allocation behind its [rows, ld] view change?  (0-dim bool tensor)"""
        n = self.rows * self.ld
        return (_bits(self.raw_out16[n:]) != _bits(self.raw_prev16[n:])).any()

    def resid(self, kind):
        return None if kind == 0 else self.r32 if kind in (1, 3) else self.r16


def scatter_of(f, g):
    """(rpg, radd, roff) of a form: the identity, or rows m -> m + m / g + 1."""
    return (g, 1, 1) if f.scatter else (INT_MAX, 0, 0)


def buffer_rows(M, g):
    """Rows of every output / residual buffer: the scattered launch's last store row + 1 and 2 rows of slack."""
    return M + (M - 1) // g + 2 + 2


def expected_of(acc, bias, f, g, bufs, prev):
    rpg, radd, roff = scatter_of(f, g)
    return reference(acc[:, :f.N], bias=bias[:f.N] if f.bias else None, alpha=f.alpha, act=f.act, resid_kind=f.resid_kind,
                     resid=bufs.resid(f.resid_kind), rpg=rpg, radd=radd, roff=roff, prev=prev)


def dense_problem(M, n_max, dev, K=K_DENSE, cin=None):
    """x ~ N(0, 1) [M + 2, ldx] (ldx = cin or K; 2 rows of slack: rows of ldx < K elements overlap the next row against zero
    weights, as the pointwise convolutions run), w ~ N(0, 0.1) [n_max, K] (columns >= cin zero), bias ~ N(0, 1), all bf16-valued;
    acc fp64 [M, n_max].  A case with N < n_max uses the first N weight rows."""
    cin = K if cin is None else cin
    x = rnd(M + 2, cin, seed=1, dtype=BF, dev=dev)
    w = torch.zeros(n_max, K, dtype=BF, device=dev)
    w[:, :cin] = rnd(n_max, cin, seed=2, scale=0.1, dtype=BF, dev=dev)
    bias = rnd(n_max, seed=3, dev=dev)
    acc = x[:M].double() @ w[:, :cin].double().t()
    return x, w, bias, acc


# ---- descriptors ------------------------------------------------------------------------------------------------------------
def fill_epilogue(d, f, g, bufs, bias, out):
    """The epilogue half of a descriptor for form f (every pointer real)."""
    d.out, d.out_kind = out.data_ptr(), 1 if f.out_f32 else 0
    d.bias = bias.data_ptr() if f.bias else None
    r = bufs.resid(f.resid_kind)
    d.resid = r.data_ptr() if r is not None else None
    d.N, d.ldo, d.ldr = f.N, bufs.ld, bufs.ld
    d.act, d.resid_kind, d.alpha = f.act, f.resid_kind, f.alpha
    d.rpg, d.radd, d.roff = scatter_of(f, g)
    d.wg_cap = f.wg_cap
    return d


def rejected_descriptors():
    """(label, descriptor) pairs msclip_gemm_variant must call "invalid" -- asked, never launched (the pointers are dummies)."""
    from msclip_amd import hip
    conv = (14, 14, 64, 14, 14, 1, 1)

    def dense(**kw):
        d = hip.describe_gemm(0, 300, 264, 128, tile=kw.pop("tile", 0), resid_kind=kw.pop("resid_kind", 0))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def conv_desc(tile, **geo):
        c = dict(zip(("H", "Wd", "Cin", "Ho", "Wo", "stride", "pad"), conv))
        c.update(geo)
        return hip.describe_gemm(1, 2 * 14 * 14, 96, 576, tile=tile, conv=tuple(c[k] for k in ("H", "Wd", "Cin", "Ho", "Wo", "stride", "pad")))

    for tile in (0, 1, 4, 6):
        for rk in (1, 2, 3):
            yield f"tile {tile}: resid_kind {rk} without resid", dense(tile=tile, resid_kind=rk, resid=None)
        for act in (-1, 3):
            yield f"tile {tile}: act {act}", dense(tile=tile, act=act)
        yield f"tile {tile}: ldo = N - 4", dense(tile=tile, ldo=260)
        for name in ("Ho", "Wo", "stride"):
            yield f"tile {tile}: mode 1 with {name} = 0", conv_desc(tile, **{name: 0})
    d = hip.describe_gemm(0, 4099, 96, 128, tile=5, resid_kind=1)
    d.resid = None
    yield "stream shape: resid_kind 1 without resid", d


def launch(d, f8_scales=None):
    """msclip_gemm / msclip_gemm_f8 on the current stream -> return code."""
    from msclip_amd import hip
    if f8_scales is not None:
        return hip.lib().msclip_gemm_f8(ctypes.byref(d), hip._p(f8_scales[0]), hip._p(f8_scales[1]), hip._stream())
    return hip.lib().msclip_gemm(ctypes.byref(d), hip._stream())
