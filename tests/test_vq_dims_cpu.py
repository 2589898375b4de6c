"""CPU suite for quantizer code widths other than 32: the constructor's width rule and the width-aware workspace query."""
import os

import pytest

WIDTHS = [8, 16, 24, 48, 64, 128, 256]


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("rq", [False, True])
def test_vector_quantizer_constructs_at_every_supported_width(d, rq):
    from enhancing.modules.stage1.quantizers import VectorQuantizer
    kw = dict(use_residual=True, num_quantizers=4) if rq else {}
    q = VectorQuantizer(d, 1024, **kw)
    assert q.embed_dim == d and tuple(q.embedding.weight.shape) == (1024, d)
    assert q.depth == (4 if rq else 1)


@pytest.mark.parametrize("d", [0, 12, 33, 264])
def test_unsupported_width_is_refused_at_construction(d):
    from enhancing.modules.stage1.quantizers import VectorQuantizer
    with pytest.raises(ValueError, match="embed_dim % 8 == 0 and 8 <= embed_dim <= 256"):
        VectorQuantizer(d, 1024)


def test_workspace_query_per_width():
    from enhancing import _C
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as G
        G.build()
    L = _C.lib()
    assert hasattr(L, "enh_vq_workspace_bytes_d") and "enh_vq_workspace_bytes_d" in _C.SIGNATURES
    for M, K, depth in [(131072, 8192, 1), (131072, 8192, 4), (1000, 500, 8)]:
        assert L.enh_vq_workspace_bytes_d(M, K, 32, depth) == L.enh_vq_workspace_bytes(M, K, depth)
        sizes = [L.enh_vq_workspace_bytes_d(M, K, d, depth) for d in [8, 16, 24, 32, 40, 48, 64, 128, 256]]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # the backward's per-(token, depth) contribution vectors dominate at wide codes: >= 1 GiB at M = 131072, depth 8, d = 256
    assert L.enh_vq_workspace_bytes_d(131072, 8192, 256, 8) >= 131072 * 8 * 256 * 4
