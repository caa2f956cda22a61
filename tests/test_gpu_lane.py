"""The lane stream's hand-offs (hip.forked; gradgemm.wgrad_async / WgradJob / on_lane) against the synchronous path: the same
kernels issued on the calling stream (options.TRAIN.wgrad_sync), which the whole-model gradient tests tie to autograd of the
reference.  Values only, bitwise; the shapes are the smallest ones the kernel tests (test_gpu_train.py) already run."""
import pytest
import torch

from msclip_amd import gradgemm, hip, options

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _operand(rows, cols, seed, scale=1.0):
    """Seeded bf16 [rows, cols]; `scale` keeps a column's sum over the rows finite and well inside fp32."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cols, generator=g) * scale).to(BF).cuda()


def _sync_then_lane(monkeypatch, dev, job):
    """job() once with the lane switched off, once with the default; -> both results, the lane's joined and complete."""
    with monkeypatch.context() as m:
        m.setattr(options, "TRAIN", options.TRAIN.replace(wgrad_sync=True))
        assert not gradgemm.lane_enabled()
        want = job()
    assert gradgemm.lane_enabled()
    got = job()
    gradgemm.join(dev)
    torch.cuda.synchronize()
    return want, got


def test_wgrad_job_wide_token_major(gpu_device, monkeypatch):
    """WgradJob on whole 256-channel tiles: nothing to do until finish(), then the token-major split-K GEMM with 2 slices."""
    dy, x = _operand(4096, 768, 1, 0.5), _operand(4096, 768, 2)
    want, got = _sync_then_lane(monkeypatch, gpu_device, lambda: gradgemm.WgradJob(dy, x, 4096).finish())
    assert got.shape == (768, 768) and bool(torch.isfinite(got).all()) and torch.equal(got, want)


@pytest.mark.parametrize("rows,n,k", [(4096, 96, 448),        # narrow, transposing: gemm_splitk with 4 slices
                                      (66000, 48, 448)])      # narrow, token-major (65 536 rows and more)
def test_wgrad_async_narrow(gpu_device, monkeypatch, rows, n, k):
    dy, x = _operand(rows, n, 3, 0.5), _operand(rows, k, 4)
    want, got = _sync_then_lane(monkeypatch, gpu_device, lambda: gradgemm.wgrad_async(dy, x, rows))
    assert got.shape == (n, k) and bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_wgrad_async_callable_operand_with_post(gpu_device, monkeypatch):
    """The operand built on the lane (a convolution's column matrix in the training step) and a post step on the result."""
    dy, x = _operand(4096, 96, 3, 0.5), _operand(4096, 448, 4)
    want, got = _sync_then_lane(monkeypatch, gpu_device, lambda: gradgemm.wgrad_async(
        dy, lambda: x, 4096, post=lambda d: d[:, :440].contiguous()))
    assert got.shape == (96, 440) and torch.equal(got, want)
    plain = gradgemm.wgrad(dy, x, 4096)
    assert torch.equal(got, plain[:, :440])


def test_on_lane(gpu_device, monkeypatch):
    a = _operand(3000, 768, 5)
    want, got = _sync_then_lane(monkeypatch, gpu_device, lambda: gradgemm.on_lane(lambda: hip.colsum(a), a))
    assert got.shape == (768,) and bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_forked_orders_the_side_stream_behind_the_current_one(gpu_device):
    """The body runs on `side` behind what the current stream had queued; the yielded object is the stream that was current,
    which is current again afterwards."""
    side = gradgemm.lane(gpu_device)
    before = torch.cuda.current_stream(gpu_device)
    src = _operand(3000, 768, 6).float()
    dst = torch.zeros(3000, 768, device=gpu_device)
    made = src * 2.0 + 1.0                                   # produced on the current stream just before the hand-off
    with hip.forked(side, made) as cur:
        assert cur == before and torch.cuda.current_stream(gpu_device) == side
        dst.copy_(made)
    assert torch.cuda.current_stream(gpu_device) == before
    before.wait_stream(side)
    assert torch.equal(dst, src * 2.0 + 1.0)
