"""The loss of the reference's training step differentiated by torch.autograd in float64 on the CPU: an independent check
of tests/_learner.py::gradient, which is a hand-derived backward pass, and through it of the kernels.

main/impl/dqn.py:238-249 (the custom-gradient step), 262-292 (the four target strategies) and 301-311 (the 5-64-64-3
network) are restated here with the reference's own array shapes and nothing derived by hand: the online forward on s, a
[B,3] `targets` array = Q(s) with column a assigned r + not done * gamma * f, the one-hot mask and the sum that keeps its
dimension ([B,1]), the subtraction, the mean, torch.autograd.grad.

  executed=True   the subtraction as written: [B,1] - [B,3] broadcasts, the mean runs over 3 B elements
  executed=False  `targets` sliced to its column a ([B,1]) first: the textbook mean squared TD error

The reference's "fixed" and "standard" strategies assign into an eager tensor, which TensorFlow refuses; they are restated
with a numpy copy, as its "double" strategy does.  "double_ref" is that strategy as it executes (arg-max of Q(s)), "double"
what its comment says (arg-max of Q(s')).  No tests/_learner.py formula is used: only its sample gathering is shared.
"""
import numpy as np

SHAPES = ((5, 64), (64, 64), (64, 3))


def _leaves(torch, theta, requires_grad):
    """the canonical vector -> [k0, b0, k1, b1, k2, b2] float64 tensors"""
    theta = np.asarray(theta, dtype=np.float32).astype(np.float64)
    out, at = [], 0
    for i, o in SHAPES:
        for shape in ((i, o), (o,)):
            n = int(np.prod(shape))
            out.append(torch.tensor(theta[at:at + n].reshape(shape), dtype=torch.float64, requires_grad=requires_grad))
            at += n
    assert at == theta.shape[0]
    return out


def _model(torch, leaves):
    k0, b0, k1, b1, k2, b2 = leaves

    def net(x):
        a1 = torch.relu(x @ k0 + b0)
        a2 = torch.relu(a1 @ k1 + b1)
        return a2 @ k2 + b2
    return net


def gradient(theta, theta_target, ring, eff, gamma, strategy, executed=True):
    """the arguments of tests/_learner.py::gradient -> (g float64 [4739] in canonical order, loss)"""
    import torch
    sel = np.asarray(eff)[np.asarray(eff) >= 0].astype(np.int64)
    size = sel.shape[0]
    if size == 0:
        return np.zeros(sum(i * o + o for i, o in SHAPES)), 0.0
    x = torch.tensor(ring["s"][:, sel].T.astype(np.float64))
    x2 = torch.tensor(ring["s2"][:, sel].T.astype(np.float64))
    act = ring["a"][sel].astype(np.int64)
    rew = ring["r"][sel].astype(np.float64)
    done = ring["d"][sel] != 0
    variables = _leaves(torch, theta, True)
    q_online = _model(torch, variables)
    q_target = _model(torch, _leaves(torch, theta_target, False))
    rows = np.arange(size)

    # the target strategy: numpy in, numpy out, nothing on the tape
    with torch.no_grad():
        if strategy == "double_ref":
            pick = np.argmax(q_online(x).numpy(), axis=1)
            f = q_target(x2).numpy()[rows, pick]
        elif strategy == "double":
            pick = np.argmax(q_online(x2).numpy(), axis=1)
            f = q_target(x2).numpy()[rows, pick]
        elif strategy == "fixed":
            f = np.max(q_target(x2).numpy(), axis=1)
        else:
            assert strategy == "standard", strategy
            f = np.max(q_online(x2).numpy(), axis=1)
        targets = q_online(x).numpy().copy()
    targets[rows, act] = rew + np.where(done, 0.0, gamma * f)
    T = torch.tensor(targets)                                  # [B, 3], a constant
    if not executed:
        T = T[rows, act].reshape(size, 1)                      # [B, 1]

    masked = q_online(x) * torch.nn.functional.one_hot(torch.tensor(act), 3).to(torch.float64)
    pred = torch.sum(masked, dim=1, keepdim=True)              # [B, 1]
    sq = (pred - T) ** 2                                       # [B, 3] as executed, else [B, 1]
    assert tuple(sq.shape) == (size, 3 if executed else 1)
    objective = sq.mean()
    grads = torch.autograd.grad(objective, variables)
    return np.concatenate([g.numpy().reshape(-1) for g in grads]), float(objective.detach())
