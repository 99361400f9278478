"""FrameRenderer: render(mode="rgb_array") for a batch of worlds, drawn on the device.

Reference being replaced: gym_aqua/envs/aqua.py:215-365, one pyglet viewer per env object, and what it keeps between
step() and render(): the thrusts and the ICC of the last action (aqua.py:151-174).  Here one kernel launch draws the
frames of M worlds as uint8 [M][S][S][3] (include/aqua_render.h has the scene), and one small launch ahead of the step
records thrusts and ICC per world.  There is no CPU path: without a HIP device or libaqua_render.so this raises.

    fr = FrameRenderer(env, size=500)
    fr.before_step(action)                 # the tensor handed to env.step(): uint8 [>=N] or float32 [2][>=N]
    obs, rew, term = env.step(action)
    frames = fr.render()                   # uint8 [min(N, 16), S, S, 3] on the device
"""
import numpy as np

from . import _render_capi

DEFAULT_WORLDS = 16


class FrameRenderer(object):
    """Frames of a BatchedAqua's worlds.  Everything is queued on torch's current stream and nothing is read back, so
    before_step() + env.step() + render() can be captured in one torch.cuda.graph.

    Restarts do not touch the overlay: a world that restarted since the last before_step() (auto_reset, or reset()) is
    drawn at its new pose with the thrust bars and the ICC of the step that ended its episode, until the next
    before_step().  Before the first before_step() there are no bars and the ICC sits at the origin, as in the reference
    after its constructor and reset()."""

    def __init__(self, env, size=500):
        torch = env.torch
        size = int(size)
        if size % 4 != 0 or not _render_capi.MIN_SIZE <= size <= _render_capi.MAX_SIZE:
            raise ValueError("size=%d: the frame side must be a multiple of 4 in [%d, %d]" % (size, _render_capi.MIN_SIZE, _render_capi.MAX_SIZE))
        if env.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("FrameRenderer draws on an AMD GPU through HIP only; there is no CPU path")
        tables = env.obstacle_tables if env.per_world else env.obstacle_rows
        if tables.shape[-2] > _render_capi.MAX_ROWS:
            raise ValueError("%d obstacle rows: the renderer draws at most %d" % (tables.shape[-2], _render_capi.MAX_ROWS))
        self.env, self.size = env, size
        self.K = int(tables.shape[-2])
        self._rows = torch.from_numpy(np.ascontiguousarray(tables, dtype=np.float32)).to(env.device) if self.K else None
        self.overlay = torch.zeros((_render_capi.OVERLAY_ROWS, env.ld), dtype=torch.float32, device=env.device)
        self._recorded = False             # until the first before_step() the frames are drawn without an overlay

    def before_step(self, action):
        """Record thrusts and ICC of the step about to be taken from the pose as it is now.  action: what
        ReplayRing.before_step() accepts: uint8 [>=N] (discrete worlds) or float32 [2][>=N] with unit inner stride."""
        e, torch, lib = self.env, self.env.torch, _render_capi.lib
        if not isinstance(action, torch.Tensor) or action.device != e.device:
            raise ValueError("the action must be a tensor on %s" % (e.device,))
        with torch.cuda.device(e.device):
            if e.continuous:
                if action.dim() != 2 or action.shape[0] != 2 or action.dtype != torch.float32 or action.shape[1] < e.num_envs \
                        or (action.shape[1] > 1 and action.stride(1) != 1):
                    raise ValueError("continuous actions are recorded from a float32 [2][>=N] tensor")
                _render_capi.check(lib.aquarnd_overlay_f32x2(e.state.data_ptr(), e.ld, e.num_envs, action.data_ptr(), action.stride(0),
                                                             self.overlay.data_ptr(), e.ld, e._stream()), "aquarnd_overlay_f32x2")
            else:
                if action.dtype != torch.uint8 or action.dim() != 1 or action.numel() < e.num_envs or not action.is_contiguous():
                    raise ValueError("discrete actions are recorded from a uint8 [>=N] tensor")
                _render_capi.check(lib.aquarnd_overlay_u8(e.state.data_ptr(), e.ld, e.num_envs, action.data_ptr(),
                                                          self.overlay.data_ptr(), e.ld, e._stream()), "aquarnd_overlay_u8")
        self._recorded = True

    def set_overlay(self, overlay):
        """Overwrite the recorded overlay (teacher forcing in tests, as BatchedAqua.set_state()): float [N][4] rows of
        (tl, tr, icc_x, icc_y)."""
        e, torch = self.env, self.env.torch
        o = torch.as_tensor(np.asarray(overlay, dtype=np.float32)) if not isinstance(overlay, torch.Tensor) else overlay
        if tuple(o.shape) != (e.num_envs, _render_capi.OVERLAY_ROWS):
            raise ValueError("overlay must be [N][4]")
        self.overlay[:, :e.num_envs].copy_(o.to(device=e.device, dtype=torch.float32).t())
        self._recorded = True

    def render(self, worlds=None, out=None):
        """-> uint8 [M, S, S, 3] on the device: the frames of worlds[...] (an int32 device tensor; an entry outside [0, N) gives
        a black frame), by default of the first min(N, 16) worlds.  out: a tensor of that shape to draw into."""
        e, torch, S = self.env, self.env.torch, self.size
        if worlds is None:
            M, wptr = min(e.num_envs, DEFAULT_WORLDS), None
        else:
            if not isinstance(worlds, torch.Tensor) or worlds.dtype != torch.int32 or worlds.dim() != 1 or worlds.device != e.device \
                    or not worlds.is_contiguous():
                raise ValueError("worlds must be a contiguous int32 [M] tensor on %s" % (e.device,))
            M, wptr = int(worlds.numel()), worlds.data_ptr()
        if out is None:
            out = torch.empty((M, S, S, 3), dtype=torch.uint8, device=e.device)
        elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (M, S, S, 3) or out.dtype != torch.uint8 or out.device != e.device \
                or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 [%d, %d, %d, 3] tensor on %s" % (M, S, S, e.device))
        with torch.cuda.device(e.device):
            _render_capi.check(_render_capi.lib.aquarnd_frames_u8(
                e.state.data_ptr(), e.ld, e.num_envs, self.overlay.data_ptr() if self._recorded else None, e.ld,
                self._rows.data_ptr() if self._rows is not None else None, self.K, int(e.per_world), int(e.has_waves),
                wptr, M, S, out.data_ptr(), out.numel(), e._stream()), "aquarnd_frames_u8")
        return out
