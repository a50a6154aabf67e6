"""The GPU R-MAT generator (stract_amd/csrc/hb_synth_gpu.hip) against the host one (hb_synth.cpp): a plain bench run loads the
graph DeviceRmatGraph builds, the --full run and the tests the graph RmatGraph builds, so both must be the same graph and
produce the same record stream, bit for bit."""
import numpy as np
import pytest

from stract_amd import _lib, synth

pytestmark = pytest.mark.gpu


def _same_graph(scale, m_target, seed=synth.SEED):
    h = synth.RmatGraph(scale, m_target, seed=seed)
    d = synth.DeviceRmatGraph(scale, m_target, seed=seed)
    try:
        assert (d.n, d.m, d.raw_drawn) == (h.n, h.m, h.raw_drawn), (scale, m_target)
        ids, row_ptr, src = d.host_arrays()
        assert np.array_equal(ids.view(np.uint64), h.ids.view(np.uint64))
        assert np.array_equal(row_ptr, h.row_ptr) and np.array_equal(src, h.src)
        for salt in (0, 2):
            total = h.stream_len(salt)
            assert d.stream_len(salt) == total
            for first, count in ((0, total), (total // 3, 1000), (max(total - 17, 0), 64)):
                a = np.zeros(count, _lib.EDGE)
                b = np.zeros(count, _lib.EDGE)
                k = h.stream_fill(a, first, salt)
                assert d.stream_fill(b, first, salt) == k
                assert a[:k].tobytes() == b[:k].tobytes(), (scale, m_target, salt, first)
    finally:
        d.close()
        h.close()


@pytest.mark.parametrize("scale,m_target", [(14, 100_000), (17, 1_000_000), (12, 30_000)])
def test_device_rmat_is_the_host_graph(scale, m_target):
    _same_graph(scale, m_target)


def test_device_rmat_draws_further_rounds_like_the_host():
    # 512 vertices' worth of R-MAT cannot give 40 000 unique edges in the first 17/16 m draws: several rounds
    h = synth.RmatGraph(9, 40_000)
    rounds_needed = h.raw_drawn > 40_000 + 40_000 // 16 + 64
    h.close()
    assert rounds_needed
    _same_graph(9, 40_000)
    _same_graph(10, 50_000, seed=7)


def test_device_config_graph_matches_make_config():
    made = synth.make_config_on_device("C1")
    g, scale, label = made
    h, hs, hl = synth.make_config("C1")
    assert (scale, label, g.n, g.m) == (hs, hl, h.n, h.m)
    g.close()
    h.close()
    assert synth.make_config_on_device("LT") is None  # the tail variant: host generator only
