"""The serial tail of the forward step on a real MI355X: the small-M GEMM kernel behind the "dense128" choice
(csrc/gemm_skinny.hip; MSCLIP_GEMM_SKINNY=0 keeps the 128 x 128 kernel) and the lane-parallel msclip_clip_loss_from_partials.

Bounds are the suite's own: the small dense launches of tests/test_gpu_kernels.py (bf16 out: 2e-2 + 1e-2 |ref|, fp32 out and the
fp32 residual update: 2e-3 + 1e-4 |ref|) and test_fused_lse_and_loss' 2e-3 for the loss and its per-row log-sum-exp."""
import pytest
import torch

from msclip_amd import hip

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def close(got, ref, atol, rtol=0.0):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    assert bool((err <= tol).all()), f"max err {err.max().item():.4g} (ref absmax {ref.abs().max().item():.4g})"


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# (M, N, K, form): plain = bias, fp32 out; gelu = bias, QuickGELU, bf16 out; resid = bias, fp32 residual updated in place;
# strided = ldx = 2K, ldo = N + 64, ldr = N + 32, alpha = 0.5, no bias, fp32 residual
CASES = [
    (1, 64, 64, "plain"), (37, 66, 64, "plain"), (65, 72, 128, "plain"), (200, 64, 64, "plain"),   # ragged M / N, N % 4 != 0, K < ring
    (64, 64, 192, "plain"), (1024, 768, 768, "plain"),                                          # q-proj / out_proj
    (1024, 3072, 768, "gelu"),                                                                  # c_fc
    (1024, 768, 3072, "resid"),                                                                 # c_proj: the ring wraps 12 times
    (512, 512, 768, "plain"),                                                                   # heads
    (128, 768, 768, "strided"),
]


def run_case(M, N, K, form):
    """-> (the output rows, the whole output buffer, reference, (atol, rtol))"""
    x = rnd(M, 2 * K if form == "strided" else K, seed=1, dtype=BF)
    w, b = rnd(N, K, seed=2, scale=0.05, dtype=BF), rnd(N, seed=3)
    base = x[:, :K].float() @ w.float().t()
    if form == "plain":
        buf = torch.full((M + 2, N), NAN, dtype=torch.float32, device="cuda")
        hip.gemm(x, w, buf[:M], bias=b)
        return buf[:M], buf, base + b, (2e-3, 1e-4)
    if form == "gelu":
        buf = torch.full((M + 2, N), NAN, dtype=BF, device="cuda")
        hip.gemm(x, w, buf[:M], bias=b, act=hip.ACT_QUICKGELU)
        v = base + b
        return buf[:M], buf, v * torch.sigmoid(1.702 * v), (2e-2, 1e-2)
    if form == "resid":
        r32 = rnd(M, N, seed=4)
        buf = torch.full((M + 2, N), NAN, dtype=torch.float32, device="cuda")
        buf[:M] = r32
        hip.gemm(x, w, buf[:M], bias=b, resid=buf[:M], resid_kind=hip.RESID_F32)
        return buf[:M], buf, r32 + base + b, (2e-3, 1e-4)
    rbuf = rnd(M, N + 32, seed=4)
    buf = torch.full((M + 2, N + 64), NAN, dtype=torch.float32, device="cuda")
    hip.gemm(x[:, :K], w, buf[:M, :N], resid=rbuf[:, :N], resid_kind=hip.RESID_F32, alpha=0.5)
    return buf[:M, :N], buf, rbuf[:, :N] + 0.5 * base, (2e-3, 1e-4)


@pytest.mark.parametrize("M,N,K,form", CASES, ids=[f"{m}x{n}x{k}-{f}" for m, n, k, f in CASES])
def test_small_m_gemm(gpu_device, monkeypatch, M, N, K, form):
    assert hip.gemm_variant(hip.describe_gemm(0, M, N, K, resid_kind=hip.RESID_F32 if form in ("resid", "strided") else 0)) == "dense128"
    outs = []
    for switch in ("1", "1", "0"):
        monkeypatch.setenv("MSCLIP_GEMM_SKINNY", switch)
        out, buf, ref, (atol, rtol) = run_case(M, N, K, form)
        err = (out.float() - ref).abs()
        print(f"switch {switch}: max err {err.max().item():.3g}, worst err / tol {(err / (atol + rtol * ref.abs())).max().item():.3g}")
        close(out, ref, atol, rtol)
        assert bool(torch.isnan(buf[M:].float()).all())                        # nothing written past M ...
        assert bool(torch.isnan(buf[:, N:].float()).all())                     # ... or past N inside a wider row
        outs.append(out.clone())
    assert torch.equal(bits(outs[0]), bits(outs[1]))                           # run to run: the same bits


def test_launches_the_small_m_kernel_does_not_carry_fall_through(gpu_device, monkeypatch):
    """A row scatter with a table residual (rpg = 49) and a bf16 residual stay with the 128 x 128 kernel: the switch changes nothing."""
    B, g2, D = 3, 49, 256
    x, w = rnd(B * g2, D, seed=9, dtype=BF), rnd(D, D, seed=10, scale=0.05, dtype=BF)
    pos = rnd(g2 + 1, D, seed=11)
    M, N, K = 333, 256, 192
    x2, w2, b2, r16 = rnd(M, K, seed=4, dtype=BF), rnd(N, K, seed=5, scale=0.08, dtype=BF), rnd(N, seed=6), rnd(M, N, seed=8, dtype=BF)
    got = []
    for switch in ("1", "0"):
        monkeypatch.setenv("MSCLIP_GEMM_SKINNY", switch)
        X = torch.zeros(B * (g2 + 1), D, dtype=torch.float32, device="cuda")
        hip.gemm(x, w, X, M=B * g2, resid=pos, resid_kind=hip.RESID_TABLE, rpg=g2, radd=1, roff=1)
        o16 = torch.empty(M, N, dtype=BF, device="cuda")
        hip.gemm(x2, w2, o16, bias=b2, resid=r16, resid_kind=hip.RESID_BF16)
        got.append((X, o16))
    assert torch.equal(bits(got[0][0]), bits(got[1][0])) and torch.equal(bits(got[0][1]), bits(got[1][1]))
    ref = (x.float() @ w.float().t()).reshape(B, g2, D) + pos[1:]
    close(got[0][0].reshape(B, g2 + 1, D)[:, 1:], ref, 2e-3, 1e-4)
    close(got[0][1], x2.float() @ w2.float().t() + b2 + r16.float(), 2e-2, 1e-2)


@pytest.mark.parametrize("nsplit", [1, 2, 8])
@pytest.mark.parametrize("R", [1, 255, 512])
def test_loss_from_partials(gpu_device, R, nsplit):
    """(max, sum-exp) partials of random logits, `nsplit` column ranges of 16; row 0's ranges have maxima > 80 apart and the last
    row's last range is empty (max -inf, sum 0: what msclip_clip_lse_fused leaves for a split without columns).  Against fp64."""
    W = 16
    lg = [rnd(R, nsplit, W, seed=60 + d, scale=6.0).double() for d in range(2)]
    for l in lg:
        if nsplit > 1:
            l[0, 0] += 100.0
    empty = nsplit > 1
    part = torch.empty(4, R, nsplit, dtype=torch.float32, device="cuda")
    lse = []
    for d, l in enumerate(lg):
        pm = l.max(2).values
        ps = torch.exp(l - pm[..., None]).sum(2)
        flat = l.reshape(R, nsplit * W).clone()
        if empty:
            pm[R - 1, nsplit - 1], ps[R - 1, nsplit - 1] = -float("inf"), 0.0
            flat[R - 1, (nsplit - 1) * W:] = -float("inf")
        part[2 * d], part[2 * d + 1] = pm.float(), ps.float()
        lse.append(torch.logsumexp(flat, 1))
    if nsplit > 1:
        assert float(part[0][0].max() - part[0][0].min()) > 80.0
    diag = rnd(R, seed=62, scale=3.0)
    scale = 1.0 / (2 * nsplit * W)
    ref = ((lse[0] - diag.double()) + (lse[1] - diag.double())).sum() * scale
    out = torch.full((1,), NAN, dtype=torch.float32, device="cuda")
    lse_out = torch.full((2, R), NAN, dtype=torch.float32, device="cuda")
    hip.clip_loss_from_partials(part[0], part[1], part[2], part[3], diag, scale, out, lse_out)
    print(f"loss err {abs(float(out[0]) - float(ref)):.3g}, lse err {(lse_out.double() - torch.stack(lse)).abs().max().item():.3g}")
    assert bool(((lse_out.double() - torch.stack(lse)).abs() <= 2e-3).all())
    assert abs(float(out[0]) - float(ref)) <= 2e-3
    again = torch.empty_like(out)
    hip.clip_loss_from_partials(part[0], part[1], part[2], part[3], diag, scale, again)      # no lse_out; run to run the same bits
    assert torch.equal(bits(out), bits(again))
