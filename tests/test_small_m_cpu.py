"""No GPU: the small-M kernel is a choice inside the "dense128" variant, not a variant of its own (bench.py and hip.py count
launches by these names)."""
import pytest

from msclip_amd import hip


@pytest.mark.parametrize("M,N,K,resid_kind", [(1024, 768, 768, 0), (1024, 768, 3072, hip.RESID_F32), (512, 512, 768, 0)])
def test_small_m_launches_keep_the_dense128_name(M, N, K, resid_kind):
    assert hip.gemm_variant(hip.describe_gemm(0, M, N, K, resid_kind=resid_kind)) == "dense128"
