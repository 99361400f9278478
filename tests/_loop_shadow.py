"""One iteration of DQNLoop / PopulationLoop (aquaticgymenv_amd/trainer.py) on the host, composed from the numpy models the
suite already holds every library to, for tests/test_loop_shadow_cpu.py and tests/test_loop_shadow_gpu.py.

    expected = shadow(before, observed, config)        differences(expected, after) -> [names]

`before` and `after` are dicts of numpy copies of the device state either side of one loop.step() (initial_state() documents
the keys, shapes and dtypes; a DQNLoop is a population of one network whose segment is the batch).  The order of the stages
is written from the class docstrings of trainer.py and the reference's loop (main/impl/dqn.py:147-184: act epsilon-greedily,
step, append, improve, move the target, and only then count the episode), not from _queue:

    act (, explore)  open  step  close  [insert]  track  [account]  [select]  draw  [relabel | fold]  update  [set]  [refresh]  tick

  - the priority insert follows the ring close and precedes the draw; the selector precedes the draw, so a replaced network
    trains on its parent's weights in that iteration; the fold reads the hyper table as the selector left it; set() gets the
    draw's slots; the relabel is keyed by the learners' t before the update advances it; refresh() follows the update and the
    selector's copy; the tick advances last.

Teacher forcing.  Two things are taken from `observed` (the state after the step): the environment's own outputs of the step
(reward, term, time, the new observation: the oracle parity tests own them; here the ring must have recorded exactly them),
and the device's grad and td, each held to the float64 model first (4 E, E the error of the same model in float32: the bar of
tests/test_prio_gpu.py::test_weighted_update_on_float_networks_against_float64 and tests/test_learner_forms_gpu.py) and then
used, so that Adam, the soft update, the blobs and the leaves set() writes are compared as tightly as their own tests do.
Where a world's two best Q-values tie within rounding (near_tie) either action is right: the device's is taken.  Without an
`observed` entry (the synthetic runs of the CPU tests) the model's own value stands in.

order=: one of ORDERS, for the tests only -- the same iteration with exactly one stage out of place.
"""
import numpy as np

from tests import _episodes as EP
from tests import _fastpol as F
from tests import _her_model as HER
from tests import _lbank as K
from tests import _learner as L
from tests import _nstep_model as NS
from tests import _pbt as PBT
from tests import _prio_model as PR
from tests import _replay as R
from tests import _segments as SG

U = 2.0 ** -24                      # tests/test_learner_gpu.py: half a unit in the last place of a float32 in [1, 2)
PARAMS = L.PARAMS
ROWS = ("s", "a", "r", "s2", "d", "ok")

# name -> (the stage that moves, where, the stage it moves next to); "set_staged" moves nothing: set() gets nstep.idx
_MOVES = {"select_after_update": ("select", "after", "update"), "insert_after_draw": ("insert", "after", "draw"),
          "refresh_before_update": ("refresh", "before", "update"), "relabel_after_update": ("relabel", "after", "update"),
          "account_before_track": ("account", "before", "track"), "select_after_fold": ("select", "after", "fold"),
          "open_before_act": ("open", "before", "act"), "explore_after_open": ("explore", "after", "open"),
          "tick_first": ("tick", "before", "act")}
ORDERS = ("set_staged",) + tuple(_MOVES)


# the variants both test files run, and the variants every order of ORDERS is tried on
VARIANTS = {"population-full": dict(kind="population", segments=True, selector=True, actor=True, n_step=2, priorities=True),
            "population-priorities": dict(kind="population", segments=True, selector=True, priorities=True),
            "population-hindsight": dict(kind="population", segments=True, selector=True, hindsight=True),
            "population-plain": dict(kind="population"),
            "dqn-actor-nstep": dict(kind="dqn", actor=True, n_step=3),
            "dqn-hindsight": dict(kind="dqn", hindsight=True),
            "dqn-plain": dict(kind="dqn")}
MUTANTS = [("set_staged", "population-full"), ("select_after_update", "population-full"), ("insert_after_draw", "population-full"),
           ("refresh_before_update", "population-full"), ("refresh_before_update", "dqn-actor-nstep"),
           ("relabel_after_update", "population-hindsight"), ("relabel_after_update", "dqn-hindsight"),
           ("account_before_track", "population-full"), ("select_after_fold", "population-full"),
           ("open_before_act", "population-plain"), ("open_before_act", "dqn-plain"), ("explore_after_open", "dqn-plain"),
           ("tick_first", "population-plain"), ("tick_first", "dqn-plain")]
# launches per stage, for the kernel counts the class docstrings of trainer.py state
LAUNCHES = dict(act=1, explore=1, open=1, step=1, close=1, insert=1, track=2, account=1, select=2, draw=1, relabel=1, fold=1, update=2,
                set=1, refresh=1, tick=1)


def config(kind, N, P, seg, B, capacity, env_seed, n_step=1, actor=False, segments=None, selector=None, priorities=None, hindsight=None,
           dqn_eps=None, env_offset=0, strategy="double_ref", loss="mse", tracker_capacity=None):
    """what shadow() needs to know of a loop: kind "population" | "dqn"; segments: None or dict(window, final [P], factor [P]);
    selector: None or dict(score, fraction, ready, every, seed, lr_factors, lr_bounds, gamma_factors, gamma_bounds); priorities:
    None or dict(alpha, beta0, anneal, eps); hindsight: None or dict(horizon, ratio); dqn_eps: (init, final, decay factor)"""
    assert kind in ("population", "dqn") and (kind == "population" or (P == 1 and seg >= N))
    return dict(kind=kind, N=N, P=P, seg=seg, B=B, capacity=capacity, env_seed=env_seed, env_offset=env_offset, n_step=n_step, actor=actor,
                segments=segments, selector=selector, priorities=priorities, hindsight=hindsight, dqn_eps=dqn_eps, strategy=strategy,
                loss=loss, tracker_capacity=max(N, 65536) if tracker_capacity is None else tracker_capacity)


def launches(config):
    """kernels of one iteration: a prioritised draw is two launches"""
    return sum(LAUNCHES[s] for s in stages(config)) + (1 if config.get("priorities") else 0)


def stages(config, order=None):
    """the stage names of one iteration of this configuration, in stream order; order: None or one of ORDERS (a ValueError
    if the configuration has no such stage)"""
    c = config
    s = ["act"] + ([] if c["kind"] == "population" else ["explore"]) + ["open", "step", "close"]
    s += ["insert"] if c.get("priorities") else []
    s += ["track"]
    s += ["account"] if c.get("segments") else []
    s += ["select"] if c.get("selector") else []
    s += ["draw"]
    s += ["relabel"] if c.get("hindsight") else (["fold"] if c["n_step"] > 1 else [])
    s += ["update"]
    s += ["set"] if c.get("priorities") else []
    s += ["refresh"] if c.get("actor") else []
    s += ["tick"]
    if order is None:
        return s
    if order == "set_staged":
        if "set" not in s or "fold" not in s:
            raise ValueError("set_staged needs priorities and n_step > 1")
        return s
    what, where, anchor = _MOVES[order]
    if what not in s or anchor not in s:
        raise ValueError("%s: this configuration has no %s or no %s stage" % (order, what, anchor))
    s.remove(what)
    s.insert(s.index(anchor) + (where == "after"), what)
    return s


# ------------------------------------------------------------------------------------------------ what an entry of `expected` can be
class Within(object):
    """|after - centre| <= bound, element by element (bound 0: the centre's bits); unit: the E the bound is a multiple of"""

    def __init__(self, centre, bound, dtype, unit=None):
        self.centre, self.bound, self.dtype, self.unit = np.asarray(centre, np.float64), np.asarray(bound, np.float64), np.dtype(dtype), unit

    def holds(self, got):
        got = np.asarray(got)
        if got.dtype != self.dtype or got.shape != self.centre.shape:
            return False
        return bool((np.abs(got.astype(np.float64) - self.centre) <= self.bound).all())

    def multiple(self, got):
        """the largest |after - centre| in units of E (0 where E is 0 and the values agree)"""
        err = np.abs(np.asarray(got).astype(np.float64) - self.centre)
        unit = np.broadcast_to(np.asarray(self.unit, np.float64), err.shape)
        ratio = np.where(unit > 0, err / np.where(unit > 0, unit, 1.0), np.where(err > 0, np.inf, 0.0))
        return float(ratio.max()) if ratio.size else 0.0


class OneOf(object):
    """after == first or after == second, element by element"""

    def __init__(self, first, second):
        self.first, self.second = np.asarray(first), np.asarray(second)

    def holds(self, got):
        got = np.asarray(got)
        if got.dtype != self.first.dtype or got.shape != self.first.shape:
            return False
        return bool(((got == self.first) | (got == self.second)).all())


def differences(expected, after, stats=None):
    """names of the entries of `after` that are not what `expected` says (bit for bit unless the entry is a Within or a
    OneOf; a callable entry is evaluated on `after` first).  stats: a dict receiving the largest multiple of E per Within"""
    bad = list(expected.get("_problems", ()))
    for name, want in expected.items():
        if name.startswith("_"):
            continue
        if name not in after:
            bad.append(name + " (missing)")
            continue
        got = after[name]
        if callable(want) and not isinstance(want, (Within, OneOf)):
            want = want(after)
        if isinstance(want, (Within, OneOf)):
            if not want.holds(got):
                bad.append(name)
            if stats is not None and isinstance(want, Within) and want.unit is not None and got.shape == want.centre.shape:
                stats[name] = max(stats.get(name, 0.0), want.multiple(got))
        elif got.dtype != want.dtype or got.shape != want.shape or got.tobytes() != np.ascontiguousarray(want).tobytes():
            bad.append(name)
    return bad


# ------------------------------------------------------------------------------------------------ the act stage
def near_tie(q64, E, factor=4.0):
    """q64 float64 [n][3] -> (exempt bool [n], best [n], second [n]): a world whose two largest float64 Q-values lie within
    factor * E of each other is exempt from the arg-max comparison; best takes the lowest index on an exact tie"""
    order = np.argsort(-q64, axis=1, kind="stable")
    rows = np.arange(q64.shape[0])
    best, second = order[:, 0], order[:, 1]
    return (q64[rows, best] - q64[rows, second]) <= factor * E, best.astype(np.uint8), second.astype(np.uint8)


def greedy(theta32, x32, fast):
    """the greedy action of one network on x32 float32 [n][5] -> (first uint8 [n], second uint8 [n], exempt bool [n]).
    float32 path: E = max |forward32 - forward64| over this batch, exempt within 4 E.  fast: the split-f16 model of
    tests/_fastpol.py, and check_contract's rule as it stands -- outside 8 E_s of a tie the float64 arg-max, inside it the
    model's pick if that is one of the two best"""
    q64 = L.forward(theta32.astype(np.float64), x32.astype(np.float64))[2]
    if not fast:
        q32 = L.forward(theta32, x32)[2]
        assert q32.dtype == np.float32
        exempt, best, second = near_tie(q64, float(np.max(np.abs(q32.astype(np.float64) - q64))))
        return best, second, exempt
    qm = F.model(L.unflatten(theta32), x32)
    E_s = float(np.max(np.abs(qm.astype(np.float64) - q64)))
    exempt, best, second = near_tie(q64, E_s, 8.0)                   # _fastpol.near_tie_share: (top - next) <= 8 E_s
    pick = np.argmax(qm, axis=1).astype(np.uint8)
    first = np.where(exempt & ((pick == best) | (pick == second)), pick, best).astype(np.uint8)
    return first, np.where(first == best, second, best).astype(np.uint8), exempt


# ------------------------------------------------------------------------------------------------ the trees as bytes
def tree_levels(raw, lay, P):
    out = []
    for k in range(lay["levels"]):
        n, stride, off = lay["n"][k], lay["stride"][k], lay["offset"][k]
        dtype = np.uint32 if k == 0 else np.uint64
        out.append(raw[off:off + P * stride * np.dtype(dtype).itemsize].view(dtype).reshape(P, stride)[:, :n].copy())
    return out


def tree_bytes(trees):
    """the buffer aquaprio_layout describes, from a _prio_model.Trees: its leaves, the exact sums above them, zero padding"""
    lay, P = trees.lay, trees.P
    raw = np.zeros(lay["bytes"], dtype=np.uint8)
    for k, level in enumerate(trees.levels()):
        stride, off = lay["stride"][k], lay["offset"][k]
        rows = np.zeros((P, stride), dtype=np.uint32 if k == 0 else np.uint64)
        rows[:, :level.shape[1]] = level
        raw[off:off + rows.nbytes] = rows.view(np.uint8).reshape(-1)
    return raw


def _pack(theta32):
    from aquaticgymenv_amd import _policy_capi
    return np.ascontiguousarray(_policy_capi.pack_weights(L.unflatten(np.ascontiguousarray(theta32, dtype=np.float32)))).view(np.uint8).reshape(-1)


def _fast_pack(theta32):
    from aquaticgymenv_amd import _fastpol_capi
    return np.ascontiguousarray(_fastpol_capi.pack_host(_pack(theta32))).view(np.uint8).reshape(-1)


# ------------------------------------------------------------------------------------------------ the state, from the constructors' documented shapes
def initial_state(config, layers, hyper6, seeds, epsilon, seed=0):
    """The state a freshly constructed loop of this configuration holds, on the host: layers: P layer stacks; hyper6: float64
    [P][6] (gamma, tau, lr, beta1, beta2, eps); seeds: the P keys of the learners; epsilon: the P (or one) initial epsilons.
    The observation row is random (an env after reset() holds its first observation), everything else is what the
    constructors write."""
    from aquaticgymenv_amd import _lbank_capi
    c = config
    N, P, B, cap, C = c["N"], c["P"], c["B"], c["capacity"], c["tracker_capacity"]
    ld = -(-N // 64) * 64
    rng = np.random.RandomState(seed)
    z = lambda shape, dt: np.zeros(shape, dtype=dt)                                           # noqa: E731
    st = {"tick": z(1, np.int64), "env.obs_norm": z((5, ld), np.float32), "env.reward": z(ld, np.float32), "env.term": z(ld, np.uint8),
          "env.time": z(ld, np.int32), "env.policy_action": z(ld, np.uint8), "ring.header": z(4, np.int64)}
    st["env.obs_norm"][:, :N] = (rng.rand(5, N) * 2 - 1).astype(np.float32)
    for name, shape, dt in (("s", (5, cap), np.float32), ("a", cap, np.uint8), ("r", cap, np.float32), ("s2", (5, cap), np.float32),
                            ("d", cap, np.uint8), ("ok", cap, np.uint8)):
        st["ring." + name] = z(shape, dt)
    st.update({"tracker.ret": z(N, np.float32), "tracker.len": z(N, np.int32), "tracker.log_ret": z(C, np.float32),
               "tracker.log_len": z(C, np.int32), "tracker.log_code": z(C, np.uint8), "tracker.log_world": z(C, np.int64),
               "tracker._counts": z(8, np.int64)})
    eps = np.asarray(epsilon, dtype=np.float64).reshape(-1)
    if c["kind"] == "dqn":
        st["tracker._eps_state"], st["tracker.epsilon"] = eps[:1].copy(), eps[:1].astype(np.float32)
    else:
        st["bank.epsilon"] = eps.astype(np.float32)
    theta = np.stack([L.flatten(x) for x in layers]).astype(np.float32)
    blobs = np.stack([_pack(th) for th in theta])
    st.update({"bank.tensor": blobs, "learners.theta": theta, "learners.theta_target": theta.copy(), "learners.m": z((P, PARAMS), np.float32),
               "learners.v": z((P, PARAMS), np.float32), "learners.t": z(P, np.int64), "learners.target_tensor": blobs.copy(),
               "learners.hyper": _lbank_capi.pack_hyper(np.asarray(hyper6, dtype=np.float64)), "learners.loss": z(P, np.float32),
               "learners.grad": z((P, PARAMS), np.float32), "learners.seed_dev": np.array(seeds, dtype=np.uint64).view(np.int64)})
    if c.get("segments"):
        W = c["segments"]["window"]
        st.update({"segments.header": z(4, np.int64), "segments._counts": z((P, 8), np.int64), "segments.win_ret": z((P, W), np.float32),
                   "segments.win_len": z((P, W), np.int32), "segments.win_code": z((P, W), np.uint8), "segments.mean_return": z(P, np.float32),
                   "segments.mean_length": z(P, np.float32), "segments.success_rate": z(P, np.float32), "segments._eps_state": eps.copy()})
    if c.get("selector"):
        st.update({"selector.header": z(4, np.int64), "selector.mark": z(P, np.int64), "selector.origin": np.arange(P, dtype=np.int32),
                   "selector.parent": np.arange(P, dtype=np.int32)})
    if c.get("priorities"):
        lay = PR.layout(cap, N, min(c["seg"], N), P)
        st.update({"per.tree": z(lay["bytes"], np.uint8), "per.pmax": np.full(P, PR.ONE, dtype=np.int32), "per.idx": np.full((P, B), -1, np.int32),
                   "per.weight": z((P, B), np.float32), "per.td": np.full((P, B), -1.0, np.float32)})
    else:
        st["loop.idx"] = np.full((P, B), -1, np.int32)
    staged = [("s", (5, P * B), np.float32), ("a", P * B, np.uint8), ("r", P * B, np.float32), ("s2", (5, P * B), np.float32),
              ("d", P * B, np.uint8), ("ok", P * B, np.uint8)]
    if c["n_step"] > 1:
        for name, shape, dt in staged + [("length", P * B, np.uint8)]:
            st["nstep." + name] = z(shape, dt)
        if c["kind"] == "population":
            st["nstep.hyper"] = z((P, 8), np.float64)
    if c.get("hindsight"):
        for name, shape, dt in staged + [("k", P * B, np.uint8), ("m", P * B, np.uint8)]:
            st["her." + name] = z(shape, dt)
    if c.get("actor"):
        st["actor.tensor"] = np.stack([_fast_pack(th) for th in theta])
    return st


# ------------------------------------------------------------------------------------------------ one iteration
class _Iteration(object):
    def __init__(self, before, observed, config, order):
        self.c, self.obs, self.order = config, ({} if observed is None else observed), order
        self.w = {k: np.array(v, copy=True) for k, v in before.items()}
        w = self.w
        self.alt = {k: w[k].copy() for k in ("env.policy_action", "ring.a")}            # the other action of a near tie
        self.exempt = np.zeros(config["N"], dtype=bool)
        self.tol = {k: np.zeros(w[k].shape, np.float64) for k in ("learners.theta", "learners.m", "learners.v")}
        self.c64 = {}
        self.special, self.problems = {}, []
        self.new_slots = np.zeros(0, dtype=np.int64)
        self.info = dict(exempt=0, replaced=0, perturbed=0, dropped_kept=0, fresh_drawn=0, relabelled=0, wrapped=False, updated=0)
        self.draw_key = "per.idx" if config.get("priorities") else "loop.idx"

    # -- helpers
    def _ring(self):
        w, m = self.w, R.Model(self.c["capacity"])
        m.header = w["ring.header"]
        for name in ROWS:
            setattr(m, name, w["ring." + name])
        return m

    def _ring_dict(self):
        out = {name: self.w["ring." + name] for name in ROWS}
        out["capacity"] = out["size"] = self.c["capacity"]               # the learner view: size = capacity
        return out

    def _trees(self):
        c, w = self.c, self.w
        t = PR.Trees(c["capacity"], c["N"], min(c["seg"], c["N"]), c["P"])
        t.leaves[:] = tree_levels(w["per.tree"], t.lay, c["P"])[0]
        t.pmax[:] = w["per.pmax"].view(np.uint32)
        return t

    def _store_trees(self, t):
        self.w["per.tree"], self.w["per.pmax"] = tree_bytes(t), t.pmax.view(np.int32).copy()

    def _seeds(self):
        return [int(x) for x in self.w["learners.seed_dev"].view(np.uint64)]

    # -- the stages
    def act(self):
        c, w = self.c, self.w
        N, P, seg = c["N"], c["P"], c["seg"]
        x = np.ascontiguousarray(w["env.obs_norm"][:, :N].T)
        tick = int(w["tick"][0])
        u, drawn = EP.draws_vectorised(N, c["env_seed"], c["env_offset"], tick)
        first, second = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
        self.exempt = np.zeros(N, dtype=bool)
        for p in range(P):
            lo, hi = p * seg, min(N, (p + 1) * seg)
            if lo >= hi:
                continue
            theta = w["learners.theta"][p]
            if w["bank.tensor"][p].tobytes() != _pack(theta).tobytes():
                self.problems.append("bank.tensor (before: not the packing of theta)")
            if c.get("actor") and w["actor.tensor"][p].tobytes() != _fast_pack(theta).tobytes():
                self.problems.append("actor.tensor (before: not the split of theta)")
            first[lo:hi], second[lo:hi], self.exempt[lo:hi] = greedy(theta, x[lo:hi], bool(c.get("actor")))
            if c["kind"] == "population":                            # the bank explores in its own launch, network p with epsilon[p]
                eps = w["bank.epsilon"][p]
                first[lo:hi], explored = EP.explore(first[lo:hi], eps, u[lo:hi], drawn[lo:hi])
                second[lo:hi] = np.where(explored, drawn[lo:hi], second[lo:hi])
                self.exempt[lo:hi] &= ~explored
        w["env.policy_action"][:N], self.alt["env.policy_action"][:N] = first, second
        self.alt["env.policy_action"][N:] = w["env.policy_action"][N:]
        if c["kind"] == "population":
            self._settle_ties()

    def explore(self):
        c, w = self.c, self.w
        N = c["N"]
        u, drawn = EP.draws_vectorised(N, c["env_seed"], c["env_offset"], int(w["tick"][0]))
        eps = w["tracker.epsilon"][0]
        w["env.policy_action"][:N], explored = EP.explore(w["env.policy_action"][:N], eps, u, drawn)
        self.alt["env.policy_action"][:N] = np.where(explored, drawn, self.alt["env.policy_action"][:N])
        self.exempt = self.exempt & ~explored
        self._settle_ties()

    def _settle_ties(self):
        """an exempt world took one of its two best actions: the device's choice stands from here on"""
        N = self.c["N"]
        a, b = self.w["env.policy_action"], self.alt["env.policy_action"]
        self.exempt &= a[:N] != b[:N]
        self.info["exempt"] = int(self.exempt.sum())
        keep = np.ones(len(a), dtype=bool)
        keep[:N] = self.exempt
        b[~keep] = a[~keep]
        got = self.obs.get("env.policy_action")
        if got is not None:
            swap = keep & (got == b) & (got != a)
            a[swap], b[swap] = b[swap], a[swap]

    def open(self):
        c, w, ring = self.c, self.w, self._ring()
        base = int(ring.header[R.CURSOR])
        ring.open(w["env.obs_norm"], w["env.policy_action"], w["env.time"], c["N"])
        if 0 <= base < c["capacity"]:
            self.new_slots = ring.slots(base, c["N"])
            self.alt["ring.a"][self.new_slots] = self.alt["env.policy_action"][:c["N"]]

    def step(self):
        for name in ("env.reward", "env.term", "env.time", "env.obs_norm", "env.state", "env.done_bits"):
            if name in self.w and name in self.obs:
                self.w[name] = np.array(self.obs[name], copy=True)

    def close(self):
        c, w, ring = self.c, self.w, self._ring()
        base = int(ring.header[R.BASE])
        ring.close(w["env.reward"], w["env.obs_norm"], w["env.term"], c["N"])
        self.info["wrapped"] = base + c["N"] >= c["capacity"]

    def insert(self):
        t = self._trees()
        t.insert(int(self.w["ring.header"][R.BASE]), self.w["ring.ok"])
        self._store_trees(t)

    def track(self):
        c, w = self.c, self.w
        N = c["N"]
        m = EP.Model(N, c["tracker_capacity"], eps=c.get("dqn_eps"))
        for name in ("ret", "len", "log_ret", "log_len", "log_code", "log_world"):
            setattr(m, name, w["tracker." + name])
        m.counts = w["tracker._counts"].view(np.uint64)
        if m.eps is not None:
            m.eps_state = float(w["tracker._eps_state"][0])
        m.after_step(w["env.reward"][:N], w["env.term"][:N], w["env.time"][:N], env_offset=c["env_offset"])
        if m.eps is not None:
            w["tracker._eps_state"][0], w["tracker.epsilon"][0] = m.eps_state, m.eps_out

    def account(self):
        c, w, s = self.c, self.w, self.c["segments"]
        m = SG.Model(c["N"], c["seg"], c["P"], s["window"], c["env_offset"], eps=(s["final"], s["final"], s["factor"]))
        m.header, m.counts = w["segments.header"].view(np.uint64), w["segments._counts"].view(np.uint64)
        m.win_ret, m.win_len, m.win_code = w["segments.win_ret"], w["segments.win_len"], w["segments.win_code"]
        m.mean_ret, m.mean_len, m.success = w["segments.mean_return"], w["segments.mean_length"], w["segments.success_rate"]
        m.eps_state, m.eps_out = w["segments._eps_state"], w["bank.epsilon"]
        m.account(w["tracker.log_ret"], w["tracker.log_len"], w["tracker.log_code"], w["tracker.log_world"],
                  int(w["tracker._counts"].view(np.uint64)[0]))

    def select(self):
        c, w, s = self.c, self.w, self.c["selector"]
        P = c["P"]
        m = PBT.Model(P, w["bank.tensor"].shape[1] // 4, fraction=s["fraction"], ready=s["ready"], every=s["every"], seed=s["seed"],
                      lr_factors=s["lr_factors"], lr_bounds=s["lr_bounds"], gamma_factors=s["gamma_factors"], gamma_bounds=s["gamma_bounds"])
        m.header, m.mark = w["selector.header"].view(np.uint64), w["selector.mark"].view(np.uint64)
        m.origin, m.parent = w["selector.origin"], w["selector.parent"]
        m.theta, m.theta_target, m.m, m.v = w["learners.theta"], w["learners.theta_target"], w["learners.m"], w["learners.v"]
        m.t = w["learners.t"].view(np.uint64)
        m.blob_online, m.blob_target = w["bank.tensor"].view(np.float32), w["learners.target_tensor"].view(np.float32)
        m.hyper, m.eps_state, m.eps_out = w["learners.hyper"], w["segments._eps_state"], w["bank.epsilon"]
        table = w["learners.hyper"].copy()
        m.select(w["segments." + {"mean_return": "mean_return", "success_rate": "success_rate"}[s["score"]]], w["segments._counts"].view(np.uint64))
        for p in m.losers:
            q = int(m.parent[p])
            self.info["replaced"] += 1
            self.info["perturbed"] += int(w["learners.hyper"][p, 0] != table[q, 0])
            for k in self.tol:                                       # (only when the selection follows the update: an order of the tests)
                self.tol[k][p] = self.tol[k][q]
                if k in self.c64:
                    self.c64[k][p] = self.c64[k][q]

    def draw(self):
        c, w = self.c, self.w
        N, P, B, cap = c["N"], c["P"], c["B"], c["capacity"]
        t, seeds = [int(x) for x in w["learners.t"]], self._seeds()
        filled = min(max(int(w["ring.header"][R.SIZE]), 0), cap)
        if c.get("priorities"):
            pr = c["priorities"]
            from aquaticgymenv_amd import _prio_capi
            trees = self._trees()
            seg = trees.seg
            for p in range(P):
                idx, q = PR.draw(trees.leaves[p], trees.lay["n"], seeds[p], t[p], B, p, N, seg, cap)
                T = int(trees.leaves[p].astype(np.uint64).sum(dtype=np.uint64))
                size_p = max(1, filled // N * PR.worlds(N, seg, p))
                w["per.idx"][p] = idx
                w["per.weight"][p] = PR.weights(q, T, size_p, _prio_capi.beta(t[p], pr["beta0"], pr["anneal"]), _prio_capi.weight)
        elif c["kind"] == "population":
            w["loop.idx"][:] = K.draw_model(seeds, t, B, filled, w["ring.ok"], cap, N, c["seg"])
        else:
            ring = self._ring_dict()
            ring["size"] = filled
            w["loop.idx"][0] = L.drawn(seeds[0], t[0] + 1, B, ring)
        idx = w[self.draw_key]
        self.info["fresh_drawn"] = int(np.isin(idx, self.new_slots).sum())

    def fold(self):
        c, w = self.c, self.w
        pop = c["kind"] == "population"
        out = NS.fold(self._ring_dict(), w["ring.header"], c["N"], w[self.draw_key], c["n_step"],
                      gamma=None if pop else float(w["learners.hyper"][0, 0]), hyper=w["learners.hyper"] if pop else None)
        for name in ROWS:
            w["nstep." + name] = out[name]
        w["nstep.length"] = out["len"]
        if pop:
            w["nstep.hyper"] = out["hyper"]

    def relabel(self):
        c, w, h = self.c, self.w, self.c["hindsight"]
        out = HER.relabel(self._ring_dict(), w["ring.header"], c["N"], w[self.draw_key], h["horizon"], h["ratio"],
                          [int(x) for x in w["learners.t"]], self._seeds())
        for name in ROWS + ("k", "m"):
            w["her." + name] = out[name]
        self.info["relabelled"] = int((out["k"] > 0).sum())

    def update(self):
        c, w, obs = self.c, self.w, self.obs
        P, B = c["P"], c["B"]
        staged = "her." if c.get("hindsight") else ("nstep." if c["n_step"] > 1 else None)
        if staged is None:
            view, idx, table = self._ring_dict(), w[self.draw_key], w["learners.hyper"]
        else:
            view = {name: w[staged + name] for name in ROWS}
            view["size"] = P * B
            idx = np.arange(P * B, dtype=np.int32).reshape(P, B)
            table = w["learners.hyper"]
            if staged == "nstep.":                                   # gamma^n: the fold's table, or DQNLoop's argument by value
                table = w["nstep.hyper"] if c["kind"] == "population" else NS.derived_table(w["learners.hyper"], c["n_step"])
        per = bool(c.get("priorities"))
        g_c, g_b, g_u = np.zeros((P, PARAMS)), np.zeros((P, PARAMS)), np.zeros((P, 1))
        l_c, l_b, l_u = np.zeros(P), np.zeros(P), np.zeros(P)
        td_c, td_b, td_u = np.full((P, B), -1.0), np.zeros((P, B)), np.zeros((P, 1))
        for k in self.tol:
            self.c64[k] = w[k].astype(np.float64)
            self.tol[k][:] = 0
        target_before = w["learners.theta_target"].copy()
        updated = np.zeros(P, dtype=bool)
        taus = np.zeros(P)
        for p in range(P):
            gamma, tau, lr, b1, b2, eps = (float(x) for x in table[p, :6])
            gamma = float(np.float32(gamma))                         # include/aqua_lbank.h: rounded to float32 where the learner rounds it
            eff = L.effective(idx[p], view)
            weight = w["per.weight"][p] if per else np.ones(B, dtype=np.float32)
            r64 = PR.weighted_gradient(w["learners.theta"][p], w["learners.theta_target"][p], view, eff, weight, gamma, c["strategy"], np.float64, c["loss"])
            r32 = PR.weighted_gradient(w["learners.theta"][p], w["learners.theta_target"][p], view, eff, weight, gamma, c["strategy"], np.float32, c["loss"])
            live = eff >= 0
            if r64["n"] > 0:
                # the bar of test_prio_gpu.py::test_weighted_update_on_float_networks_against_float64 (and test_learner_forms_gpu.py): 4 E
                g_c[p], g_u[p] = r64["g"], float(np.max(np.abs(r32["g"].astype(np.float64) - r64["g"])))
                g_b[p] = 4 * g_u[p]
                l_c[p], l_u[p] = float(r64["loss"]), max(abs(float(r32["loss"]) - float(r64["loss"])), float(np.spacing(np.float32(r64["loss"]))))
                l_b[p] = 4 * l_u[p]
                td_c[p], td_u[p] = r64["td"], float(np.max(np.abs(r32["td"][live] - r64["td"][live])))
                td_b[p][live] = 4 * td_u[p] + 1e-7
            g = obs["learners.grad"][p] if "learners.grad" in obs else g_c[p].astype(np.float32)
            w["learners.grad"][p], w["learners.loss"][p] = g, (obs["learners.loss"][p] if "learners.loss" in obs else np.float32(l_c[p]))
            if per:
                w["per.td"][p] = obs["per.td"][p] if "per.td" in obs else td_c[p].astype(np.float32)
            if r64["n"] == 0:                                        # aqua_learner.h: B_eff == 0 leaves everything but loss and grad as it was
                continue
            updated[p], taus[p] = True, tau
            # Adam, the soft update and the re-pack from the device's own gradient: tests/test_learner_gpu.py::_check_step's bars
            th, m, v, t = w["learners.theta"][p], w["learners.m"][p], w["learners.v"][p], int(w["learners.t"][p])
            th64, m64, v64, t1 = L.adam64(th, w["learners.theta_target"][p], m, v, t, g, lr, tau, b1, b2, eps)
            a, g64 = (lambda z: np.abs(np.asarray(z, dtype=np.float64))), g.astype(np.float64)
            self.tol["learners.m"][p] = 3 * U * (b1 * a(m) + (1 - b1) * a(g64))
            self.tol["learners.v"][p] = 3 * U * (b2 * a(v) + (1 - b2) * g64 * g64)
            self.tol["learners.theta"][p] = U * (a(th64) + 64 * lr)
            self.c64["learners.theta"][p], self.c64["learners.m"][p], self.c64["learners.v"][p] = th64, m64, v64
            w["learners.theta"][p], w["learners.m"][p], w["learners.v"][p] = th64.astype(np.float32), m64.astype(np.float32), v64.astype(np.float32)
            w["learners.t"][p] = t1
            w["learners.theta_target"][p] = L.soft64(w["learners.theta"][p], target_before[p], tau).astype(np.float32)
            w["bank.tensor"][p], w["learners.target_tensor"][p] = _pack(w["learners.theta"][p]), _pack(w["learners.theta_target"][p])
        self.info["updated"] = int(updated.sum())
        self.special["learners.grad"] = Within(g_c, g_b, np.float32, unit=g_u)
        self.special["learners.loss"] = Within(l_c, l_b, np.float32, unit=l_u)
        if per:
            self.special["per.td"] = Within(td_c, td_b, np.float32, unit=td_u)
        kept = {k: w[k].copy() for k in ("learners.theta_target", "bank.tensor", "learners.target_tensor")}

        def target(after):
            centre, bound = kept["learners.theta_target"].astype(np.float64), np.zeros((P, PARAMS))
            for p in np.nonzero(updated)[0]:
                th = after["learners.theta"][p]
                centre[p] = L.soft64(th, target_before[p], taus[p])
                bound[p] = 3 * U * (taus[p] * np.abs(th.astype(np.float64)) + (1 - taus[p]) * np.abs(target_before[p].astype(np.float64)))
            return Within(centre, bound, np.float32)

        def blob(of, name):
            def packed(after):
                out = kept[name].copy()
                for p in np.nonzero(updated)[0]:
                    out[p] = _pack(after[of][p])
                return out
            return packed
        self.special["learners.theta_target"] = target
        self.special["bank.tensor"] = blob("learners.theta", "bank.tensor")
        self.special["learners.target_tensor"] = blob("learners.theta_target", "learners.target_tensor")

    def set(self):
        c, w = self.c, self.w
        from aquaticgymenv_amd import _prio_capi
        pr = c["priorities"]
        trees = self._trees()
        before = trees.leaves.copy()
        draw = w["per.idx"]
        idx = np.arange(c["P"] * c["B"], dtype=np.int32).reshape(c["P"], c["B"]) if self.order == "set_staged" else draw
        trees.set(idx, w["per.td"], lambda x: _prio_capi.quantise(abs(x), pr["alpha"], pr["eps"]))
        self._store_trees(trees)
        if c["n_step"] > 1:                                          # a window the fold dropped keeps its priority
            dropped = (draw >= 0) & (w["nstep.ok"].reshape(draw.shape) == 0)
            for p, j in zip(*np.nonzero(dropped)):
                owner, leaf = PR.leaf_of_slot(int(draw[p, j]), c["N"], trees.seg)
                self.info["dropped_kept"] += int(owner == p and trees.leaves[p, leaf] == before[p, leaf] and before[p, leaf] != 0)

    def refresh(self):
        w = self.w
        w["actor.tensor"] = np.stack([_fast_pack(th) for th in w["learners.theta"]])
        self.special["actor.tensor"] = lambda after: np.stack([_fast_pack(th) for th in after["learners.theta"]])

    def tick(self):
        self.w["tick"][0] += 1

    def run(self):
        for name in stages(self.c, self.order):
            getattr(self, name)()
        expected = dict(self.w)
        for k in self.tol:
            if k in self.c64:
                expected[k] = Within(self.c64[k], self.tol[k], np.float32)
        expected.update(self.special)
        for k in ("env.policy_action", "ring.a"):
            expected[k] = OneOf(self.w[k], self.alt[k])
        expected["_model"], expected["_info"], expected["_problems"] = self.w, self.info, self.problems
        return expected


def shadow(before, observed, config, order=None):
    """-> expected: for every key of `before` the array the state after one iteration must hold (or a Within, a OneOf, or a
    callable of `after` where the comparison is derived from the device's own values), "_model": the model's own next state
    (what the CPU tests iterate on), "_info": what the iteration reached."""
    return _Iteration(before, observed, config, order).run()
