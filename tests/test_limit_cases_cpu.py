"""The premises of tests/test_gpu_list_limits.py from the oracle alone: every list's largest count belongs to one frame of the
batch, the generic-path frame holds a component no flood window takes and the most candidates, the flat frame holds nothing, and
the large-list frame is the smallest of its family whose unfiltered refine output passes 1024 records."""
import numpy as np
import pytest

from tests import limit_cases as L


@pytest.fixture(scope="module")
def counts():
    return [L.oracle_counts(f) for f in L.batch()]


def test_every_largest_count_is_one_frames_alone(counts):
    assert L.unique_argmax([c["n_saddles"] for c in counts], "n_saddles") == L.I_NOISE
    assert L.unique_argmax([c["n_clusters"] for c in counts], "n_clusters") == L.I_NOISE
    assert L.unique_argmax([c["n_candidates"] for c in counts], "n_candidates") == L.I_BIG
    boards = [c["n_saddles"] for c in counts[:3]]
    assert len(set(boards)) == 3 and min(boards) > 100, boards  # the boards differ, and each is a board
    # no limit of the legs is small enough for a default floor to matter, and none is zero ("keep the default")
    assert all(c["n_saddles"] - 1 > 0 for c in counts[:5])


def test_the_generic_frame_and_the_flat_frame(counts):
    big, flat = counts[L.I_BIG], counts[L.I_FLAT]
    # a component wider and higher than the shorter side of the second-tier window (128 x 64) leaves both windows
    assert min(big["largest_extent"]) > 64, big
    assert big["n_saddles"] >= 2, big      # (a limit of n - 1 is still an explicit limit, not 0)
    assert flat == dict(n_saddles=0, n_clusters=0, n_candidates=0, n_refined=0, largest=0, largest_extent=(0, 0))
    assert not np.shares_memory(L.batch()[L.I_BIG], L.big_frame())


def test_the_large_list_frame_is_the_smallest_of_its_family():
    at, below = L.oracle_counts(L.large_frame()), L.oracle_counts(L.noise_frame(L.LARGE_BELOW_W))
    assert at["n_refined"] > 1024 >= below["n_refined"], (at, below)
    assert at["n_saddles"] <= 1024, at  # max_saddles at its bound keeps the LDS list at 1024 entries: the records sort in global memory
