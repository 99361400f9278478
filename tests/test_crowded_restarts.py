"""Restarts in crowded worlds: every re-seeding variant of the kernels where the rare branches of the placement loop
(reset_env_group, aqua_device.hpp) are the common case.

The worlds are walls that accept a candidate with p = 2 % ... 30 %, or never (tests/_placement.py), so that one wavefront
holds groups that finish in the first round of G attempts next to groups that find the goal in a later round and scan
the boat attempts serially, groups that run out of goal or boat attempts, and whole wavefronts and blocks of worlds
without any free place.  One cell per variant of the table access, chosen through the dispatch model: the shared table
(quick table / LDS-staged rows and the row loop), per-world tables of 8 ... 64 rows in both restart modes, step(),
rollout(), the fused rollout and captured graphs; a fixed goal or boat where that is a branch of its own; reset() and
reset(mask) on both sides of the switch between one world per lane and G lanes per world.

Per cell: how many worlds of each branch class it re-seeds is computed from the oracle chain alone and asserted before a
kernel output is read (tests/test_placement_cpu.py does the same on the CPU); the cell then runs through the chain
runner of tests/test_option_matrix.py (re-seeded worlds and time markers bit for bit the oracle's, live worlds within
the suite's bars, every entry point equal to the chain); and the device's own placements must satisfy the reference's
acceptance predicates, with the exemptions -- an exhausted loop leaves exactly the fixed values -- taken from the trace.
"""
import numpy as np
import pytest

from tests import _dispatch as D
from tests import _options as O
from tests import _placement as P
from tests._parity import _host_state
from tests.test_dispatch_matrix import SEED
from tests.test_option_matrix import _make, _run_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.mark.parametrize("cell", P.CELLS, ids=[P.cell_id(c) for c in P.CELLS])
def test_crowded_cell_against_the_oracle(torch, oracle, cell):
    fam, opts = cell.fam, O.OPTIONS[cell.option]
    per_world = fam.table == "world"
    # the kernels this cell is there for, by the dispatch model
    kernels = {O.strip_template(k) for k in O.family_kernels(fam)}
    if per_world:
        assert "step_tables_kernel" in kernels and D.fused_tables_kernels("u8", fam.mode, fam.K) <= O.family_kernels(fam)
    else:
        assert ("step_ns_kernel" if fam.mode == 2 else "step_kernel") in kernels and "rollout_kernel" in kernels
    # what the cell re-seeds, from the CPU side alone, before any kernel output is read
    total, per_tick, n_reseeded, stepped = P.cell_class_counts(oracle, cell)
    print("\n%s: re-seeded per tick %s  %s" % (P.cell_id(cell), n_reseeded, dict(total)))
    P.assert_cell_classes(cell, total, n_reseeded)

    inputs = P.cell_inputs(oracle, cell)
    obst = inputs[0]
    worst = [np.inf, np.inf]
    seen = []

    def observe(what, tick, k_state, k_time, reseeded):
        w, traced, ag, ab = P.trace_reseeded(cell, obst, reseeded, tick)
        assert np.array_equal(k_state[:, w].view(np.uint32), traced.view(np.uint32)), \
            "%s: %d re-seeded worlds differ from the trace" % (what, int(np.any(k_state[:, w] != traced, axis=0).sum()))
        g, b = P.check_acceptance(k_state[:, w], obst[w] if per_world else obst, ag, ab, what)
        worst[0], worst[1] = min(worst[0], g), min(worst[1], b)
        seen.append(what)

    failures = []
    _run_chain(torch, oracle, fam, opts, False, failures, inputs=inputs, observe=observe)
    print("%s: worst acceptance margin on the device: goal %+.3g  boat %+.3g  (%d states looked at)" % (
        P.cell_id(cell), worst[0], worst[1], len(seen)))
    assert not failures, "\n".join(failures)
    assert len(seen) == P.T + len(fam.entries) - 1, seen


# ------------------------------------------------------------------------------------------------ reset(), reset(mask)
RESET_N = 20000 + 333
RESET_TABLES = (("shared", 8, 2.0), ("shared", 9, 2.0), ("shared", 8, 0.0), ("world", 9, None), ("world", 33, None))
RESET_OPTIONS = ("default", "fixed_goal", "fixed_boat")
RESET_CELLS = [(t, o, d) for t in RESET_TABLES for o in (RESET_OPTIONS if t[:2] in (("shared", 8), ("world", 9)) and t[2] != 0.0
                                                         else ("default",)) for d in (0.03, 0.6)]
STATE_GUARD = -55.5


@pytest.mark.parametrize("cell", RESET_CELLS, ids=["%s-K%d-%s-%s-mask%g" % (t[0], t[1], "tables" if t[2] is None else "free%g" % t[2], o, d)
                                                   for t, o, d in RESET_CELLS])
def test_reset_and_masked_reset_in_crowded_worlds(torch, oracle, cell):
    """reset(): one world per lane (reset_env / reset_env_world).  reset(mask): the shared table one world per lane; per
    world tables G lanes per world where a block selects few worlds and one world per lane where it selects many (the
    densities of test_per_world_masked_reset_sparse_and_dense_masks_match_the_oracle, both sides of RESET_DENSE)."""
    (table, K, free), option, density = cell
    opts = O.OPTIONS[option]
    rb, rg = opts["random_boat"], opts["random_goal"]
    per_world = table == "world"
    n, off = RESET_N, 4096
    obst = P.crowded_tables(K, n, seed=5)[0] if per_world else P.crowded_rows(K, free)
    rng = np.random.RandomState(int(density * 1000) + K)
    mask = rng.uniform(size=n) < density
    scan, dense = D.C["RESET_SCAN"], D.C["RESET_DENSE"]
    per_block = np.add.reduceat(mask.astype(np.int64), np.arange(0, n, scan))
    assert np.all(per_block > dense) if density > 0.5 else np.all(per_block[:-1] <= dense) and per_block.max() >= 8
    env_ids = np.uint64(off) + np.arange(n, dtype=np.uint64)
    want_classes = P.classes_for(opts) if free != 0.0 else ("both_exhausted",)

    # the CPU side first: traces, class counts
    first = P.placement_trace(SEED, env_ids, O.RESET_TICK_BASE, obst, 1, rb, rg)
    picked = np.flatnonzero(mask)
    second = P.placement_trace(SEED, env_ids[picked], O.RESET_TICK_BASE + 1, obst[picked] if per_world else obst, 1, rb, rg)
    for what, (_, ag, ab) in (("reset()", first), ("reset(mask)", second)):
        counts = P.class_counts(ag, ab)
        print("%s: %s" % (what, dict(counts)))
        for k in want_classes:
            assert counts[k] >= (P.MIN_PER_CLASS if what == "reset()" or density > 0.5 else 1), (what, k, counts)
    reset = oracle.reset_tables if per_world else oracle.reset
    st, tt = np.zeros((7, n), dtype=np.float32), np.full(n, 5, dtype=np.int32)
    reset(st, tt, obst, waves=1, random_boat=rb, random_goal=rg, seed=SEED, tick=O.RESET_TICK_BASE, env_offset=off)
    assert np.array_equal(st.view(np.uint32), first[0].view(np.uint32))

    env = _make(torch, n, obst, False, 0, off, 1, rb, rg, O.DEFAULT_LIMIT, False)
    env.state[:, n:].fill_(STATE_GUARD)
    env.reset()
    torch.cuda.synchronize()
    k_state, k_time = _host_state(env)
    assert np.array_equal(k_state.view(np.uint32), st.view(np.uint32)) and np.array_equal(k_time, tt), "reset()"
    worst = P.check_acceptance(k_state, obst, first[1], first[2], "reset()")
    env.reset(mask=torch.as_tensor(mask).cuda())
    torch.cuda.synchronize()
    reset(st, tt, obst, waves=1, random_boat=rb, random_goal=rg, seed=SEED, tick=O.RESET_TICK_BASE + 1, env_offset=off,
          mask=mask.astype(np.uint8))
    after, after_time = _host_state(env)
    assert np.array_equal(after.view(np.uint32), st.view(np.uint32)) and np.array_equal(after_time, tt), "reset(mask)"
    assert np.array_equal(after[:, ~mask], k_state[:, ~mask]), "reset(mask) moved a world it was not given"
    assert np.array_equal(after[:, picked].view(np.uint32), second[0].view(np.uint32))
    worst2 = P.check_acceptance(after[:, picked], obst[picked] if per_world else obst, second[1], second[2], "reset(mask)")
    assert bool(torch.all(env.state[:, n:] == STATE_GUARD)), "the guard columns n .. ld were written"
    print("worst acceptance margin on the device: reset() goal %+.3g boat %+.3g, reset(mask) goal %+.3g boat %+.3g" % (
        worst + worst2))
