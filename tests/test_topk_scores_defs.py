"""embedding_ops.topk_scores without a GPU: what it supports, what it refuses before any library call, and the sizes it shares with
include/pgl_amd.h."""
import os
import re

import pytest
import torch


def test_supported_edges():
    from pgl_amd import embedding_ops as E
    assert all(E.topk_supported(d, k) for d, k in ((4, 1), (1024, 64), (8, 64), (1024, 1)))
    assert not any(E.topk_supported(d, k) for d, k in ((0, 1), (2, 1), (6, 1), (1028, 1), (8, 0), (8, 65)))


class _Index:
    indptr, col32, num_nodes = torch.zeros(9, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 8


@pytest.mark.parametrize("change", [
    {},                                                              # CPU tensors: there is no host path
    {"query": torch.zeros(3, 8, dtype=torch.float64)}, {"table": torch.zeros(10, 8, dtype=torch.float16)},
    {"query": torch.zeros(3, 6), "table": torch.zeros(10, 6)}, {"query": torch.zeros(3, 1028), "table": torch.zeros(10, 1028)},
    {"query": torch.zeros(3, 4)}, {"k": 0}, {"k": 65}, {"lo": 5, "hi": 5}, {"lo": -1}, {"hi": 11},
    {"bias": torch.zeros(9)}, {"bias": torch.zeros(10, dtype=torch.float64)},
    {"exclude": _Index()}, {"query_ids": torch.zeros(3, dtype=torch.int64)},
    {"exclude": _Index(), "query_ids": torch.zeros(3, dtype=torch.int32)}, {"slices": 0}, {"slices": 33}])
def test_refused_before_any_launch(change, monkeypatch):
    from pgl_amd import _ffi, embedding_ops as E
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was reached"))
    args = dict(query=torch.zeros(3, 8), table=torch.zeros(10, 8), k=2)
    args.update(change)
    with pytest.raises(ValueError):
        E.topk_scores(**args)
    assert E.LAUNCHES["topk_scores"] == 0


def test_sizes_shared_with_the_header():
    from pgl_amd import _ffi, embedding_ops as E
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pgl_amd.h")).read()
    assert int(re.search(r"#define PGLAMD_TOPK_MAX_K (\d+)", hdr).group(1)) == E.TOPK_MAX_K
    L = _ffi.lib()
    for Q, k, S in ((1, 1, 2), (33, 20, 3), (70, 64, 32), (100000, 20, 7)):
        assert L.pglamd_topk_scores_workspace_bytes(Q, k, 1) == 0 and L.pglamd_topk_scores_workspace_bytes(Q, k, 0) == 0
        assert L.pglamd_topk_scores_workspace_bytes(Q, k, S) >= Q * S * k * 8
        assert 1 <= L.pglamd_topk_scores_slices(Q, 1 << 20) <= E.TOPK_MAX_SLICES
    assert L.pglamd_topk_scores_slices(5, 100) == 1
