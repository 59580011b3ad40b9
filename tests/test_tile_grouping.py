"""The replay's side of tile grouping (tests/fuzz/sim_tile_regroup.py), on the CPU: the permutation it forms and the tiles it cuts from it against a
plain reference sort and a plain loop.  tests/test_tile_grouping_gpu.py holds the library's map against the same functions."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def load_sim():
    spec = importlib.util.spec_from_file_location("sim_tile_regroup", ROOT / "tests" / "fuzz" / "sim_tile_regroup.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("B", [1, 15, 16, 17, 271, 1000, 4099])
def test_replay_permutation_and_tiles_agree_with_a_plain_sort(B):
    sim = load_sim()
    rng = np.random.default_rng(B)
    start = rng.integers(0, 271, B).astype(np.int32)
    it = rng.integers(1, 100, B)
    m = sim.group_by_start(start)
    npad = (B + 15) // 16 * 16
    assert m.dtype == np.int32 and m.shape == (npad,)
    assert np.array_equal(np.sort(m[:B]), np.arange(B)) and (m[B:] == -1).all()
    assert np.array_equal(start[m[:B]], np.array(sorted(start.tolist()), np.int32))   # sorted by start ...
    for s in np.unique(start):                                                        # ... and stable inside one start
        assert (np.diff(m[:B][start[m[:B]] == s]) > 0).all()
    # tiles: sixteen consecutive entries of the map; a tile costs the largest count of the instances it serves
    want = [max(it[j] for j in m[t * 16:(t + 1) * 16] if j >= 0) for t in range(npad // 16)]
    assert np.array_equal(sim.tile_counts(it, m), np.array(want))
    assert sim.lock_step(it, m) == pytest.approx(np.mean(want) / it.mean(), rel=1e-12)
    ident = sim.identity_map(B)
    assert np.array_equal(ident[:B], np.arange(B)) and (ident[B:] == -1).all()
    assert np.array_equal(sim.tile_counts(it, ident), np.array([it[t * 16:(t + 1) * 16].max() for t in range(npad // 16)]))


def test_grouping_equal_counts_inside_a_start_reaches_lock_step_one():
    """counts that are a function of the start alone: tiles by start waste only where a tile straddles two starts, index-order tiles of a shuffled
    batch mix all of them"""
    sim = load_sim()
    rng = np.random.default_rng(3)
    start = rng.permutation(np.repeat(np.arange(64), 64)).astype(np.int32)   # 64 instances = 4 whole tiles per start
    it = 10 + start
    assert sim.lock_step(it, sim.group_by_start(start)) == pytest.approx(1.0)
    assert sim.lock_step(it, sim.identity_map(len(start))) > 1.3


def test_bucket_is_the_sorts_bucket():
    sim = load_sim()
    k = np.array([0.0, 1e-3, 0.5, 0.5625, 1.0, 3.0], np.float32)
    b = sim.bucket(k)
    assert b[0] == 0 and (np.diff(b) >= 0).all() and b[2] != b[3] and b.max() < 2048
    assert b[4] == (0x3f800000 >> 20)
