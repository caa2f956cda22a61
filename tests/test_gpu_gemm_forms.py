"""Every kernel behind msclip_gemm (and msclip_gemm_f8) over the product of the epilogue forms, on a real MI355X, against the
contract of include/msclip_hip.h as tests/gemm_forms.py states it in fp64.

Per kernel: the smallest shape with an interior tile, a ragged row tile and a ragged column tile; per form the library is ASKED
first (msclip_gemm_variant) and its answer must be what gemm_forms.promised() reads from the documentation; what it accepts is
launched once and the WHOLE output buffer compared: gemm_forms.bounds() on every stored element, every other element bit for bit
what the buffer held.  Every buffer is sized for the largest reading of it and every pointer is real, so a form routed to the
wrong epilogue branch shows as a wrong number, not as a fault.  tests/test_gemm_forms_cpu.py shows the bounds catch such a branch."""
import pytest
import torch
import torch.nn.functional as F

import gemm_forms as GF
from msclip_amd import hip, packing as P

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"

# kernel case -> (gemm_forms.promised's kernel name, msclip_gemm_variant's name, tile, MSCLIP_GEMM_SKINNY, wg_cap values)
DENSE = {
    "dense128": ("dense128", "dense128", 1, None, (0, 1)),
    "small_m": ("dense128", "dense128", 0, "1", (0,)),           # tile 0: the small-M kernel takes what it carries ...
    "small_m_off": ("dense128", "dense128", 0, "0", (0,)),       # ... and with the switch off the 128 x 128 kernel everything
    "dense192": ("dense192", "dense192", 6, None, (0, 1)),
    "pp": ("pp", "pp", 4, None, (0, 1)),
}
CONV = {
    "conv128": ("conv128", "conv128", 1, (0, 1)),
    "conv192": ("conv192", "conv192", 6, (0, 1)),
    "ppconv": ("ppconv", "ppconv", 4, (0, 1)),
}


class Tally:
    def __init__(self, name, kernel=None):
        self.kernel = kernel or name
        self.name, self.run, self.promised, self.rejected, self.elsewhere, self.worst = name, 0, 0, 0, 0, 0.0
        self.bad, self.mismatch = [], []

    def report(self):
        print(f"\n{self.name}: {self.run} forms run ({self.promised} promised), {self.rejected} rejected, {self.elsewhere} taken by "
              f"another kernel, worst err / tol {self.worst:.3g}")
        assert not self.mismatch, f"{self.name}: the library's answer is not the documented one on {len(self.mismatch)} forms, first {self.mismatch[:3]}"
        assert not self.bad, f"{self.name}: {len(self.bad)} forms outside the contract, first {self.bad[:3]}"
        assert self.run == self.promised > 0
        assert self.elsewhere == GF.ELSEWHERE.get(self.kernel, 0)         # a new silent fall-back shows here


def sweep(tally, kernel, variant, form_list, make_desc, acc, bias, g, bufs, f8_scales=None):
    """Ask, compare with the promise, launch what was accepted, check the whole buffer.  make_desc(f, out) -> descriptor."""
    pending = []
    for f in form_list:
        b = bufs[(f.N, f.ld_pad)]
        out, prev = b.out(f.out_f32)
        d = make_desc(f, out)
        want = GF.promised(kernel, f)
        tally.promised += want
        if f8_scales is None:
            name = hip.gemm_variant(d)
            if name != GF.expected_variant(kernel, f):           # a refusal, an acceptance or a fall-back nobody documented
                tally.mismatch.append((f, name, GF.expected_variant(kernel, f)))
                continue
            accepted = name == variant
            tally.rejected += name == "invalid"
            tally.elsewhere += name not in ("invalid", variant)
            rc = GF.launch(d) if accepted else None
        else:                                                    # no query for the fp8 entry: its return code is the answer
            rc = GF.launch(d, f8_scales)
            accepted = rc == 0
            tally.rejected += rc == -1                           # MSCLIP_EINVAL
        if accepted != want:
            tally.mismatch.append((f, "accepted" if accepted else "refused"))
            continue
        if not accepted:
            continue
        assert rc == 0, (f, rc)
        tally.run += 1
        expected, stored = GF.expected_of(acc, bias, f, g, b, prev)
        w = GF.worst(out, expected, stored, prev, f.resid_kind)
        if not f.out_f32:
            w = torch.where(b.slack_moved(), torch.full_like(w, float("inf")), w)
        pending.append((f, w))
    for f, w in pending:
        w = float(w)
        if not w <= 1.0:
            tally.bad.append((f, w))
        elif w > tally.worst:
            tally.worst = w


def make_bufs(M, g, n_values, seed):
    rows = GF.buffer_rows(M, g)
    return {(N, pad): GF.Buffers(rows, N + pad, DEV, seed=seed + 16 * N + pad) for N in n_values for pad in GF.LD_PADS}


def base_desc(x, w, K):
    d = hip.GemmDesc()
    d.X, d.W, d.zero = x.data_ptr(), w.data_ptr(), hip.zero_page(x.device).data_ptr()
    d.K, d.ldw = K, w.stride(0)
    return d


@pytest.mark.parametrize("case", list(DENSE))
def test_dense_kernels(gpu_device, monkeypatch, case):
    kernel, variant, tile, skinny, wg_caps = DENSE[case]
    if skinny is not None:
        monkeypatch.setenv("MSCLIP_GEMM_SKINNY", skinny)
    M, g, n_values = 300, 49, (264, 266)
    x, w, bias, acc = GF.dense_problem(M, max(n_values), DEV)
    bufs = make_bufs(M, g, n_values, seed=200)

    def make_desc(f, out):
        d = base_desc(x, w, GF.K_DENSE)
        d.mode, d.M, d.ldx, d.tile = 0, M, x.stride(0), tile
        return GF.fill_epilogue(d, f, g, bufs[(f.N, f.ld_pad)], bias, out)

    t = Tally(case, kernel)
    form_list = list(GF.forms(n_values, wg_caps))
    sweep(t, kernel, variant, form_list, make_desc, acc, bias, g, bufs)
    t.report()
    if case == "small_m":
        # Blind spot, shared with tests/test_gpu_small_m.py: msclip_gemm_variant says "dense128" whether the small-M kernel took
        # the launch or left it to the 128 x 128 kernel, and the library has no other query.  What can be said: by the documented
        # conditions (gemm_forms.small_m_takes; 3 x 3 tiles, far fewer than CUs) these forms were the small-M kernel's, the rest of
        # this case repeats small_m_off.
        mine = [f for f in form_list if GF.small_m_takes(f) and GF.promised(kernel, f)]
        print(f"small_m: {len(mine)} of the {t.run} forms are the small-M kernel's by its documented conditions")
        assert len(mine) == 2 * 3 * 2 * 2 * 2 * 2 * 2                # N x ld x bias x alpha x act 0 / 1 x resid 0 / 1 x out kind


def test_stream_dense(gpu_device):
    """tile 5 on the pointwise-convolution layout of test_gemm_streaming_small_k: K = 128 over rows of ldx = 96 elements."""
    M, g, n_values, K, cin = 4099, 49, (96, 40, 42), 128, 96
    x, w, bias, acc = GF.dense_problem(M, max(n_values), DEV, K=K, cin=cin)
    bufs = make_bufs(M, g, n_values, seed=300)

    def make_desc(f, out):
        d = base_desc(x, w, K)
        d.mode, d.M, d.ldx, d.tile = 0, M, cin, 5
        return GF.fill_epilogue(d, f, g, bufs[(f.N, f.ld_pad)], bias, out)

    t = Tally("stream")
    sweep(t, "stream", "stream", list(GF.forms(n_values)), make_desc, acc, bias, g, bufs)
    t.report()


def conv_problem(B, H, Cin, n_values, k, stride, pad):
    """NHWC x ~ N(0, 1), OIHW w ~ N(0, 0.1) (bf16-rounded by ConvSpec), bias ~ N(0, 1); acc = F.conv2d in fp64 (on the host:
    exact products, no library in between), [M, max N]; one ConvSpec per N over the first N filters."""
    nmax = max(n_values)
    x = GF.rnd(B, H, H, Cin, seed=1, dtype=BF)
    w4 = GF.rnd(nmax, Cin, k, k, seed=2, scale=0.1)
    bias = GF.rnd(nmax, seed=3, dev=DEV)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w4.to(BF).double(), stride=stride, padding=pad)
    acc = ref.permute(0, 2, 3, 1).reshape(-1, nmax).contiguous().to(DEV)
    specs = {N: P.ConvSpec(w4[:N], torch.zeros(N), H, H, stride, pad).to(DEV) for N in n_values}
    return x.to(DEV), specs, bias, acc


def conv_sweep(name, kernel, variant, tile, wg_caps, shape, n_values, seed):
    B, H, Cin, k, stride, pad = shape
    x, specs, bias, acc = conv_problem(B, H, Cin, n_values, k, stride, pad)
    s0 = specs[n_values[0]]
    g = s0.h_out * s0.w_out
    M = B * g
    assert acc.shape[0] == M
    bufs = make_bufs(M, g, n_values, seed=seed)

    def make_desc(f, out):
        s = specs[f.N]
        d = base_desc(x, s.weight, s.weight.shape[1])
        d.mode, d.M, d.tile, d.ktab = 1, M, tile, s.ktab.data_ptr()
        d.H, d.Wd, d.Cin, d.Ho, d.Wo, d.stride, d.pad = s.geometry()
        return GF.fill_epilogue(d, f, g, bufs[(f.N, f.ld_pad)], bias, out)

    t = Tally(name, kernel)
    sweep(t, kernel, variant, list(GF.forms(n_values, wg_caps)), make_desc, acc, bias, g, bufs)
    t.report()


@pytest.mark.parametrize("case", list(CONV))
def test_conv_kernels(gpu_device, case):
    kernel, variant, tile, wg_caps = CONV[case]
    conv_sweep(case, kernel, variant, tile, wg_caps, (2, 14, 64, 3, 1, 1), (96, 98), seed=400)


def test_stream_conv(gpu_device):
    """tile 5 on a 3 x 3 stride-2 convolution over 48 channels (K = 448: all of W resident in LDS; at most 96 output channels, so
    the ragged N is 94)."""
    conv_sweep("stream_conv", "stream_conv", "stream", 5, (0,), (3, 112, 48, 3, 2, 1), (96, 94), seed=500)


def _dq(q, s):
    return q.view(hip.F8).double() * s.double()[:, None]


def f8_problem(M, n_max, K):
    xq, sx = hip.quantize_rows_f8(GF.rnd(M, K, seed=1, dev=DEV))
    wq, sw = hip.quantize_rows_f8(GF.rnd(n_max, K, seed=2, scale=0.1, dev=DEV))
    return xq, sx, wq, sw, GF.rnd(n_max, seed=3, dev=DEV), _dq(xq, sx) @ _dq(wq, sw).t()


def f8_desc(xq, wq, M, K):
    d = base_desc(xq, wq, K)
    d.mode, d.M, d.ldx = 0, M, xq.stride(0)
    return d


def test_f8_entry(gpu_device):
    """msclip_gemm_f8: the product of the dequantised operands is the contraction; the header promises it msclip_gemm's bias /
    activation / residual (kinds 0 - 2) / output kinds.  There is no query for this entry: every form is launched (all buffers are
    real and sized for the scattered fp32 reading) and the return code is the library's answer."""
    M, g, n_values, K = 300, 49, (264, 266), 128
    xq, sx, wq, sw, bias, acc = f8_problem(M, max(n_values), K)
    bufs = make_bufs(M, g, n_values, seed=600)

    def make_desc(f, out):
        return GF.fill_epilogue(f8_desc(xq, wq, M, K), f, g, bufs[(f.N, f.ld_pad)], bias, out)

    t = Tally("f8")
    sweep(t, "f8", "f8", list(GF.forms(n_values, (0, 1))), make_desc, acc, bias, g, bufs, f8_scales=(sx, sw))
    t.report()


def test_f8_entry_rejects_what_it_does_not_carry(gpu_device):
    """bn_mode, `part` without xb and a tile that is neither 0 nor 4, on an otherwise valid, fully allocated launch."""
    M, N, K = 300, 264, 128
    xq, sx, wq, sw, bias, _ = f8_problem(M, N, K)
    bufs = GF.Buffers(GF.buffer_rows(M, 49), N, DEV, seed=700)
    f = GF.Form(True, 1.0, 0, 0, True, False, N, 0, 0)
    part = torch.zeros(2048, 2 * N, device=DEV)

    def rc(**kw):
        out, _ = bufs.out(True)
        d = GF.fill_epilogue(f8_desc(xq, wq, M, K), f, 49, bufs, bias, out)
        for k, v in kw.items():
            setattr(d, k, v)
        return GF.launch(d, (sx, sw))

    assert rc() == 0
    for kw in (dict(bn_mode=1, part=part.data_ptr(), part_rows=2048), dict(bn_mode=2), dict(part=part.data_ptr()),
               dict(tile=1), dict(tile=5), dict(tile=6), dict(act=3), dict(act=-1), dict(ldo=N - 4)):
        assert rc(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.equal(bufs.out32, bufs.prev32)                            # a refused launch writes nothing
    # (resid_kind without resid is NOT asked of this entry: it has no query, and the answer of a regressed check would be a
    #  kernel reading address 0.  msclip_gemm_f8 calls the same desc_ok() as msclip_gemm_variant, which is asked below.)


def test_descriptor_holes_are_rejected(gpu_device, monkeypatch):
    """Asked through msclip_gemm_variant only: no launch.  The bindings refuse a residual kind without its tensor before they
    enter the library -- shown with the library's launch entries replaced, so that a regression is a failed assertion here and
    never a kernel handed a NULL pointer."""
    for label, d in GF.rejected_descriptors():
        assert hip.gemm_variant(d) == "invalid", label
    x, w = GF.rnd(300, 128, dtype=BF, dev=DEV), GF.rnd(264, 128, scale=0.1, dtype=BF, dev=DEV)
    xq, sx, wq, sw, _, _ = f8_problem(300, 264, 128)
    out = torch.zeros(300, 264, device=DEV)
    hip.zero_page(x.device)
    entered = []

    class NoLaunch:
        def __getattr__(self, name):
            def entry(*args):
                entered.append(name)
                return -1
            return entry

    monkeypatch.setattr(hip, "lib", lambda: NoLaunch())
    for kind in (hip.RESID_F32, hip.RESID_BF16, hip.RESID_TABLE, hip.RESID_RELUMASK, hip.RESID_ACCUM):
        with pytest.raises(hip.HipError, match="without a resid tensor"):
            hip.gemm(x, w, out, resid_kind=kind)
    for kind in (hip.RESID_F32, hip.RESID_BF16):
        with pytest.raises(hip.HipError, match="without a resid tensor"):
            hip.gemm_f8(xq, wq, out, sx, sw, resid_kind=kind)
    assert not entered
