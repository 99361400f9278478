"""QValueMaps: what a Q-network has learnt, as the reference's plotter shows it
(main/plotting/dqn_qvalue_plotter.py::plot_network_qvalue): for a fixed goal the best action and the best Q-value at every
cell of the world, for a number of headings -- for every network of a bank and any number of goals in ONE launch of
libaqua_qmap.so (aquaticgymenv_amd/csrc/aqua_qmap.h).

The map is defined over four tables of normalised network inputs, xs [W], ys [H], angles [S] and goals [G][2]: the state of
network p, goal g, sector k, row r, column c is (xs[c], ys[r], angles[k], goals[g][0], goals[g][1]).  The kernel makes every
input in registers from the tables, so nothing is read per state; nothing is flipped either: the orientation of a map is the
order of the tables, and QValueMaps.reference() builds the tables that give the reference's arrays.

The object reads the policy's own device tensor (a QNetwork's blob, a slot of a bank, a whole bank) without a copy: a
later load(), learner update or selection is seen by the next call or graph replay.  There is no CPU path.
"""
import ctypes

import numpy as np

from . import _qmap_capi
from .qbank import QNetworkBank
from .qpolicy import QNetwork


class QValueMaps(object):
    def __init__(self, policy, xs, ys, angles):
        """policy: a QNetwork, a slot of a bank (bank.view(p)) or a QNetworkBank; xs [W], ys [H], angles [S]: the network's
        inputs 0, 1 and 2 by column, row and sector, already normalised (cast to float32 and copied to the policy's device)."""
        if not isinstance(policy, QNetwork):
            raise ValueError("policy must be a QNetwork, a slot of a bank or a QNetworkBank, got %r" % (type(policy).__name__,))
        self.policy, self.torch, self.device = policy, policy.torch, policy.device
        if self.device.type != "cuda":
            raise RuntimeError("QValueMaps runs on an AMD GPU through HIP only (device=%r); there is no CPU path" % (self.device,))
        if int(_qmap_capi.lib.aquaqmap_weights_bytes()) != int(policy.tensor.shape[-1] if isinstance(policy, QNetworkBank) else policy.blob.numel()):
            raise RuntimeError("libaqua_qmap.so and the policy disagree on the blob: rebuild")
        self.networks = policy.networks if isinstance(policy, QNetworkBank) else 1
        self.world_size = None
        tables = []
        for name, t, cap in (("xs", xs, _qmap_capi.MAX_SIDE), ("ys", ys, _qmap_capi.MAX_SIDE), ("angles", angles, _qmap_capi.MAX_SECTORS)):
            t = np.ascontiguousarray(np.asarray(t), dtype=np.float32)
            if t.ndim != 1 or not 1 <= t.size <= cap:
                raise ValueError("%s must be a vector of 1 .. %d network inputs, got shape %r" % (name, cap, t.shape))
            tables.append(t)
        self.W, self.H, self.S = (int(t.size) for t in tables)
        if self.S * self.H * self.W > _qmap_capi.MAX_STATES:
            raise ValueError("xs, ys, angles: %d x %d x %d states per map, more than %d" % (self.S, self.H, self.W, _qmap_capi.MAX_STATES))
        # one device tensor for the three tables: [xs | ys | angles]
        self._tables = self.torch.from_numpy(np.concatenate(tables)).to(self.device)
        self.xs, self.ys, self.angles = self._tables[:self.W], self._tables[self.W:self.W + self.H], self._tables[self.W + self.H:]

    @classmethod
    def reference(cls, policy, world_size=100, sectors=8):
        """The reference's grid (dqn_qvalue_plotter.py:12-16): cell centres (1 .. n) / n computed in float64 as :12 does,
        REVERSED for both axes (which is its flipud / fliplr, :22-23), and `sectors` headings linspace(0, 1, endpoint=False).
        maps() then divides goals by world_size as :14 does, and as_reference(action)[p, g] is its best_action."""
        maps = cls(policy, *cls.reference_tables(world_size, sectors))
        maps.world_size = int(world_size)
        return maps

    @staticmethod
    def reference_tables(world_size=100, sectors=8):
        """-> (xs, ys, angles) of reference(), float32 on the host (no device needed)"""
        n, s = int(world_size), int(sectors)
        if n < 1 or s < 1:
            raise ValueError("world_size=%r, sectors=%r: must be >= 1" % (world_size, sectors))
        coords = (np.arange(1, n + 1) / n).astype(np.float32)
        return coords[::-1].copy(), coords[::-1].copy(), np.linspace(0, 1, s, endpoint=False).astype(np.float32)

    @staticmethod
    def normalised_goals(goals, world_size=None):
        """goals [G][2] in world units -> float32 [G][2] network inputs: divided by world_size in float64 and then cast, as
        dqn_qvalue_plotter.py:14 does (world_size None: cast only); on the host"""
        g = np.asarray(goals, dtype=np.float64)
        if g.ndim != 2 or g.shape[1] != 2 or g.shape[0] < 1:
            raise ValueError("goals must be [G][2] in world units, got shape %r" % (g.shape,))
        if world_size is not None:
            g = g / world_size
        return np.ascontiguousarray(g.astype(np.float32))

    # ------------------------------------------------------------------ plumbing
    def _bank_ptr(self):
        """the policy's own device memory, asked at every call (no copy is kept)"""
        t = self.policy.tensor if isinstance(self.policy, QNetworkBank) else self.policy.blob
        return t.data_ptr()

    def _out(self, t, name, dtype, shape):
        torch = self.torch
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise ValueError("%s must be a %s tensor" % (name, str(dtype).replace("torch.", "")))
        if t.device != self.device:
            raise ValueError("%s is on %s, the policy on %s" % (name, t.device, self.device))
        if tuple(t.shape) != shape:
            raise ValueError("%s must have shape %r, got %r" % (name, shape, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
        return t

    def _goals(self, goals):
        torch = self.torch
        if isinstance(goals, torch.Tensor):
            if goals.dtype != torch.float32 or goals.dim() != 2 or goals.shape[1] != 2 or goals.shape[0] < 1 or not goals.is_contiguous():
                raise ValueError("goals as a tensor must be contiguous float32 [G][2], already normalised")
            if goals.device != self.device:
                raise ValueError("goals is on %s, the policy on %s" % (goals.device, self.device))
            return goals
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("goals must be a float32 device tensor [G][2] under graph capture (a host array would be copied)")
        return torch.from_numpy(self.normalised_goals(goals, self.world_size)).to(self.device)

    # ------------------------------------------------------------------ the path
    def maps(self, goals, action=None, value=None, q=None):
        """The maps of every network for every goal, one launch on the current stream.

        goals:  a host array [G][2] in world units, divided by world_size in float64 and then cast (maps made by
                reference(); tables given to the constructor take goals as network inputs), or a float32 device tensor [G][2],
                already normalised (the only form under graph capture).
        action: uint8 [P, G, S, H, W]; value: float32 [P, G, S, H, W]; q: float32 [P, G, 3, S, H, W], written when given.
                With none of the three, action and value are new tensors (not under capture: it writes only into tensors the
                caller passed).
        -> (action, value)"""
        torch = self.torch
        goals = self._goals(goals)
        G = int(goals.shape[0])
        if G > _qmap_capi.MAX_GOALS:
            raise ValueError("goals: %d, more than %d" % (G, _qmap_capi.MAX_GOALS))
        shape = (self.networks, G, self.S, self.H, self.W)
        action = self._out(action, "action", torch.uint8, shape)
        value = self._out(value, "value", torch.float32, shape)
        q = self._out(q, "q", torch.float32, shape[:2] + (_qmap_capi.ACTIONS,) + shape[2:])
        if action is None and value is None and q is None:
            if torch.cuda.is_current_stream_capturing():
                raise ValueError("action, value, q: pass the tensors to write into under graph capture")
            action = torch.empty(shape, dtype=torch.uint8, device=self.device)
            value = torch.empty(shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            rc = _qmap_capi.lib.aquaqmap_maps_f32(self._bank_ptr(), self.networks, self.xs.data_ptr(), self.W, self.ys.data_ptr(), self.H,
                                                  self.angles.data_ptr(), self.S, goals.data_ptr(), G,
                                                  None if action is None else action.data_ptr(), None if value is None else value.data_ptr(),
                                                  None if q is None else q.data_ptr(), stream)
        _qmap_capi.check(rc, "aquaqmap_maps_f32")
        return action, value

    @staticmethod
    def as_reference(t):
        """[..., S, H, W] -> the reference's [..., H, W, S] (a view)"""
        return t.permute(*range(t.dim() - 3), t.dim() - 2, t.dim() - 1, t.dim() - 3)
