#!/usr/bin/env python3
"""Look at an episode: a few worlds run the reference's hand-coded policy (main/testing/test_optimal.py: turn towards the
goal, then full throttle) until every one of them has ended, and the frames of one world, drawn on the device by
FrameRenderer (render(mode="rgb_array") of gym_aqua/envs/aqua.py:215-365), are written as PNGs -- or, without PIL, as one
.npy of shape [T, S, S, 3].

    python examples/render_episode.py [--envs 8] [--world 0] [--size 500] [--obstacles] [--out frames]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from aquaticgymenv_amd.batched import BatchedAqua
from aquaticgymenv_amd.render import FrameRenderer

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=8)
ap.add_argument("--world", type=int, default=0, help="the world whose frames are kept")
ap.add_argument("--size", type=int, default=500, help="frame side in pixels, a multiple of 4 (the reference: 500)")
ap.add_argument("--obstacles", action="store_true", help="the reference's default five obstacles")
ap.add_argument("--out", default="frames", help="directory of the PNGs (or the .npy)")
args = ap.parse_args()


def bearing(obs):
    """test_optimal.py on a batch: 0 turn left, 1 turn right, 2 straight -> uint8 [N] (the tensor the renderer records from)"""
    boat = torch.remainder(obs[:, 2] + math.pi / 2, 2 * math.pi)
    goal = torch.remainder(torch.atan2(obs[:, 4] - obs[:, 1], obs[:, 3] - obs[:, 0]), 2 * math.pi)
    diff = goal - boat
    turn = torch.where(diff > 0, 0, 1)
    return torch.where(diff.abs() > 8 / 180 * math.pi, turn, 2).to(torch.uint8)


env = BatchedAqua(args.envs, obstacles=args.obstacles, seed=1, auto_reset=False)
renderer = FrameRenderer(env, size=args.size)
world = torch.tensor([args.world], dtype=torch.int32, device=env.device)
obs = env.reset()
frames = [renderer.render(worlds=world)[0].cpu().numpy()]                   # the first frame: no bars yet
first = torch.zeros(args.envs, dtype=torch.uint8, device=env.device)       # first termination code of every world
for step in range(1001):
    action = bearing(obs)
    renderer.before_step(action)
    obs, reward, term = env.step(action)
    if int(first[args.world]) == 0:                                         # the kept world is still in its episode
        frames.append(renderer.render(worlds=world)[0].cpu().numpy())
    first = torch.where(first == 0, term, first)
    if int((first == 0).sum()) == 0:
        break
names = {0: "still running", 1: "collided", 2: "time limit", 3: "reached the goal"}
print("world %d: %d frames, %s" % (args.world, len(frames), names[int(first[args.world])]))
os.makedirs(args.out, exist_ok=True)
try:
    from PIL import Image
except ImportError:
    Image = None
if Image is not None:
    for t, frame in enumerate(frames):
        Image.fromarray(frame, "RGB").save(os.path.join(args.out, "frame_%04d.png" % t))
    print("wrote %d PNGs to %s" % (len(frames), args.out))
else:
    np.save(os.path.join(args.out, "frames.npy"), np.stack(frames))
    print("wrote %s" % os.path.join(args.out, "frames.npy"))
