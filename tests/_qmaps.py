"""What the tests of the Q-value maps (libaqua_qmap.so, aquaticgymenv_amd/qmaps.py) share: the reference plotter's states
restated literally (main/plotting/dqn_qvalue_plotter.py:12-16, :22-23), the composition of a map's states from its four
tables, the int64 model of a bank's maps with the mutations it must tell apart, and the split of a launch's items into the
contiguous runs of its wavefronts (the rule aquaticgymenv_amd/csrc/aqua_qmap.h documents)."""
import numpy as np

from tests._qbank import ACT_FILL, Q_FILL, family, int_eval

DEV = "cuda:0"
TILE = 32


# ------------------------------------------------------------------------------------------------ the reference's states
def plotter_states(goal, world_size, sectors=8):
    """dqn_qvalue_plotter.py:12-16, literally -> float64 [world_size^2 * sectors][5] (pos_x, pos_y, angle, goal)"""
    goal_state = np.array([goal])
    coord_per_angle = np.tile((np.arange(1, world_size + 1) / world_size).repeat(sectors), (world_size, 1))
    angles = np.tile(np.linspace([0], [1], sectors, endpoint=False), (world_size ** 2, 1))
    goal_pos = np.tile(goal_state / world_size, (sectors * world_size ** 2, 1))
    return np.concatenate((coord_per_angle.reshape([-1, 1]), coord_per_angle.transpose().reshape([-1, 1]), angles, goal_pos), axis=1)


def plotter_flips(per_state, world_size, sectors):
    """:22-23 for an array with one leading entry per state [n^2 * S, ...] -> [n][n][S][...] after flipud / fliplr"""
    return np.fliplr(np.flipud(per_state.reshape((world_size, world_size, sectors) + per_state.shape[1:])))


def composed(xs, ys, angles, goal, transposed=False):
    """the states of one map from its tables, [S][H][W][5]: (xs[c], ys[r], angles[k], goal); transposed: input 0 by row and
    input 1 by column, the assignment that does NOT reproduce the reference"""
    S, H, W = len(angles), len(ys), len(xs)
    out = np.empty((S, H, W, 5), dtype=np.asarray(xs).dtype)
    k, r, c = np.meshgrid(np.arange(S), np.arange(H), np.arange(W), indexing="ij")
    out[..., 0] = np.asarray(ys)[r] if transposed else np.asarray(xs)[c]
    out[..., 1] = np.asarray(xs)[c] if transposed else np.asarray(ys)[r]
    out[..., 2] = np.asarray(angles)[k]
    out[..., 3], out[..., 4] = goal[0], goal[1]
    return out


# ------------------------------------------------------------------------------------------------ the int64 model
def tie_layers():
    """family(0) with a zero output kernel and b2 = (4, 4, 4): every state is a three-way tie"""
    (k0, b0), (k1, b1), (k2, b2) = family(0)
    return [(k0, b0), (k1, b1), (np.zeros_like(k2), np.array([4, 4, 4], dtype=np.float32))]


MUTATIONS = ("swap_xy", "swap_goal", "sector_row", "wrong_network")


def int_maps(networks, xs, ys, angles, goals, mutation=None):
    """networks: layer stacks of small integers; tables: small integers -> Q int64 [P][G][3][S][H][W] of the map as
    aqua_qmap.h defines it.  mutation: one of MUTATIONS, a model that is wrong in that way"""
    xs, ys, angles, goals = (np.asarray(t, dtype=np.int64) for t in (xs, ys, angles, goals))
    S, H, W, G, P = len(angles), len(ys), len(xs), len(goals), len(networks)
    k, r, c = np.meshgrid(np.arange(S), np.arange(H), np.arange(W), indexing="ij")
    if mutation == "sector_row":
        row = k * H + r
        k, r = row % S, row // S
    out = np.empty((P, G, 3, S, H, W), dtype=np.int64)
    cache = {}
    for g in range(G):
        goal = goals[g][::-1] if mutation == "swap_goal" else goals[g]
        x = np.stack([xs[c], ys[r], angles[k], np.full_like(c, goal[0]), np.full_like(c, goal[1])], axis=-1).reshape(-1, 5)
        if mutation == "swap_xy":
            x = x[:, [1, 0, 2, 3, 4]]
        for p in range(P):
            layers = networks[(p + 1) % P] if mutation == "wrong_network" else networks[p]
            key = (id(layers), g)
            if key not in cache:
                cache[key] = int_eval(layers, x).T.reshape(3, S, H, W)
            out[p, g] = cache[key]
    return out


def picks(q):
    """Q [P][G][3][...] -> (action uint8, value) as the kernel picks them: np.argmax, the lowest index on a tie"""
    action = np.argmax(q, axis=2)
    return action.astype(np.uint8), np.take_along_axis(q, action[:, :, None], axis=2)[:, :, 0]


# ------------------------------------------------------------------------------------------------ the launch's split
def runs(items, compute_units):
    """-> [(first, count)] of the wavefronts of a launch, as aqua_qmap.h states the rule"""
    n = 4 * min(-(-items // 4), 3 * compute_units)
    s, t = divmod(items, n)
    return [(w * s + min(w, t), s + (1 if w < t else 0)) for w in range(n)]


def network_of(item, G, tiles):
    return item // (tiles * G)


def run_changes_network(items, compute_units, G, tiles):
    """does a change of network fall inside at least one wavefront's run?"""
    return any(count > 1 and network_of(first, G, tiles) != network_of(first + count - 1, G, tiles)
               for first, count in runs(items, compute_units))


# ------------------------------------------------------------------------------------------------ device side
def outputs(torch, P, G, S, H, W, pad=37):
    """flat sentinel-filled buffers larger than the extent, and the [P, G, ..] views a call writes into"""
    n = P * G * S * H * W
    a = torch.full((n + pad,), ACT_FILL, dtype=torch.uint8, device=DEV)
    v = torch.full((n + pad,), Q_FILL, dtype=torch.float32, device=DEV)
    q = torch.full((3 * n + pad,), Q_FILL, dtype=torch.float32, device=DEV)
    return (a, v, q), (a[:n].view(P, G, S, H, W), v[:n].view(P, G, S, H, W), q[:3 * n].view(P, G, 3, S, H, W))


def untouched(flat, P, G, S, H, W, written=(True, True, True)):
    """nothing behind the extent was written, and an output that was not asked for not at all"""
    n = P * G * S * H * W
    a, v, q = flat
    ok = bool((a[n if written[0] else 0:] == ACT_FILL).all()) and bool((v[n if written[1] else 0:] == Q_FILL).all())
    return ok and bool((q[3 * n if written[2] else 0:] == Q_FILL).all())
