"""CPU-only groundwork of tests/test_launch_regimes_gpu.py, which runs the learner, the episode accounting, the exploration
pass and the ring's draw and gather ABOVE their grid caps, where a wavefront, block or thread takes several tiles in a loop.

The GPU file derives its sizes and the placement of its samples from Python mirrors of the two `shape_of` functions
(tests/_learner.py::launch_shape, tests/_episodes.py::launch_shape).  Here the constants those mirrors use are pinned through
the libraries' public workspace functions alone, the mirrors through their values at the thresholds, the vectorised
exploration model through the per-world oracle loop, and the sparse index vectors of the exact-gradient test through the
properties they are built for and the int64 bound that makes every float32 sum exact."""
import os

import numpy as np
import pytest

from tests import _episodes as E
from tests import _learner as L

LEARNER_SIZES = (32768, 32769, 32833, 65537, 65577, 65601, 1 << 20)
EPISODE_SIZES = (262144, 262145, 524289, 524588)


@pytest.fixture(scope="module")
def lcapi():
    from aquaticgymenv_amd.build import build_learner, build_policy
    assert os.path.exists(build_policy()) and os.path.exists(build_learner())
    from aquaticgymenv_amd import _learner_capi
    return _learner_capi


@pytest.fixture(scope="module")
def ecapi():
    from aquaticgymenv_amd.build import build_episodes
    assert os.path.exists(build_episodes())
    from aquaticgymenv_amd import _episodes_capi
    return _episodes_capi


def test_learner_group_cap_from_the_workspace_function(lcapi):
    ws = lcapi.lib.aqualrn_workspace_bytes
    assert lcapi.MAX_BATCH == 1 << 20
    per_group = ws(1) - 16
    assert per_group > 4 * lcapi.PARAMS and (ws(lcapi.MAX_BATCH) - 16) % per_group == 0
    assert (ws(lcapi.MAX_BATCH) - 16) // per_group == L.GMAX == 512
    # one more group per WAVES tiles of TILE samples, until the cap
    per = L.WAVES * L.TILE
    assert ws(per) == ws(1) < ws(per + 1) == 16 + 2 * per_group
    assert ws(L.GMAX * per - per) < ws(L.GMAX * per) == ws(L.GMAX * per + 1) == ws(lcapi.MAX_BATCH)
    sizes = [ws(b) for b in sorted(LEARNER_SIZES)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    # the bound holds the partials of every launch shape used
    for B in LEARNER_SIZES:
        assert ws(B) >= 16 + L.launch_shape(B)[2] * per_group, B


def test_episode_block_cap_from_the_workspace_function(ecapi):
    ws = ecapi.lib.aquaep_workspace_bytes
    assert ecapi.MAX_BLOCKS == E.MAX_BLOCKS == 1024
    top = ws(ecapi.MAX_WORLDS)
    assert top == 4 * E.MAX_BLOCKS                                  # one uint32 per block
    assert ws(E.MAX_BLOCKS * E.BLOCK) == top == ws(E.MAX_BLOCKS * E.BLOCK + 1)
    assert ws((E.MAX_BLOCKS - 4) * E.BLOCK) < top
    assert ws(1024) < ws(1025)                                      # the fifth block begins at world 4 * 256
    assert ws(4 * E.BLOCK) == ws(1) and ws(8 * E.BLOCK) == ws(1025) < ws(8 * E.BLOCK + 1)
    sizes = [ws(n) for n in sorted(EPISODE_SIZES)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    for N in EPISODE_SIZES:
        assert ws(N) >= 4 * E.launch_shape(N)[1], N


def test_learner_launch_shape_at_its_thresholds():
    assert L.launch_shape(1) == (1, 1, 1) and L.launch_shape(4113) == (129, 1, 65)
    assert L.launch_shape(32768) == (1024, 1, 512)
    assert L.launch_shape(32769) == (1025, 2, 257)
    assert L.launch_shape(65537) == (2049, 3, 342)
    assert L.launch_shape(1 << 20) == (32768, 32, 512)
    for B in list(range(1, 3000, 7)) + list(LEARNER_SIZES):
        tiles, tpw, groups = L.launch_shape(B)
        assert 1 <= groups <= L.GMAX and groups * L.WAVES * tpw >= tiles > (groups - 1) * L.WAVES * tpw


def test_episode_launch_shape_at_its_thresholds():
    assert E.launch_shape(1) == (256, 1) and E.launch_shape(4099) == (256, 17)
    assert E.launch_shape(262144) == (256, 1024)
    assert E.launch_shape(262145) == (512, 513)
    assert E.launch_shape(524289) == (768, 683)
    assert E.launch_shape(524588) == (768, 684)                     # 683 * 768 = 524 544: 44 worlds in a block of their own
    for N in list(range(1, 5000, 13)) + list(EPISODE_SIZES):
        chunk, blocks = E.launch_shape(N)
        assert chunk % E.BLOCK == 0 and 1 <= blocks <= E.MAX_BLOCKS and blocks * chunk >= N > (blocks - 1) * chunk


@pytest.mark.parametrize("tick", [0, (1 << 32) + 5])
def test_vectorised_exploration_model_is_the_oracle_loop(oracle, tick):
    seed, off, n = 0x1234567890ABCDEF, 3 << 20, 300
    u, act = E.draws(oracle, n, seed, off, tick)
    vu, vact = E.draws_vectorised(n, seed, off, tick)
    assert vu.dtype == np.float32 and vact.dtype == np.uint8
    assert np.array_equal(vu.view(np.uint32), u.view(np.uint32)) and np.array_equal(vact, act)
    assert len(set(act.tolist())) == 3 and 0.0 <= float(u.min()) < 0.1 and 0.9 < float(u.max()) < 1.0
    # an offset beyond 32 bits reaches the second counter word
    far = (5 << 32) + 12345
    fu, fact = E.draws(oracle, 50, seed, far, tick)
    vu, vact = E.draws_vectorised(50, seed, far, tick)
    assert np.array_equal(vu, fu) and np.array_equal(vact, fact) and not np.array_equal(fu, u[:50])


@pytest.mark.parametrize("strategy", L.STRATEGIES)
@pytest.mark.parametrize("B", [32769, 65601, 1 << 20])
def test_sparse_batches_are_placed_as_promised_and_stay_exact(B, strategy):
    """the index vectors of the GPU file's exact-gradient test: the placement holds, and the largest sum of |terms| over
    every intermediate and gradient element stays below 2^24, so that float32 adds them exactly in any order"""
    cap, size = 300, 257
    ring = L.int_ring(cap, size, B % 1000, bad_ok=0.1)
    idx, plan = L.sparse_indices(B, ring, cap, seed=B % 1000 + 1)
    eff = L.check_sparse(B, idx, ring, cap, plan)
    theta, theta_t = L.flatten(L.int_layers("plain")), L.flatten(L.int_layers("plain", salt=1))
    worst, S, ref = L.abs_sums(theta, theta_t, ring, eff, strategy)
    print("B %d %s: %d valid of %d placed, largest sum of |terms| 2^%.1f" % (B, strategy, ref["n"], (idx != -1).sum(), np.log2(worst)))
    assert worst < 2 ** 24 and 1500 < ref["n"] <= L.VALID_MAX
    want = S.astype(np.float32) * np.float32(2.0 / ref["n"])
    assert np.array_equal(S.astype(np.float32).astype(np.int64), S) and np.count_nonzero(want) > 500
