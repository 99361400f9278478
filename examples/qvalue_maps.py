#!/usr/bin/env python3
"""Look at what a Q-network has learnt: main/plotting/dqn_qvalue_plotter.py's __main__ without TensorFlow or matplotlib.  For
a fixed goal, the best Q-value (scaled to grey) beside the best action (one colour per action) at every cell of the world,
one image per network and heading -- all networks in ONE launch of QValueMaps on the device.

    python examples/qvalue_maps.py [variables_dir ...] [--goal 50 50] [--world 100] [--sectors 8] [--out qvalue_maps]

variables_dir: the variables/ directories of Keras SavedModels written by dqn.py:316-321 (read through tf_import); without
any, the two policies of tests/golden/dqn_policies.npz.  PNGs with PIL, else one .npy per image.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from aquaticgymenv_amd.qbank import QNetworkBank
from aquaticgymenv_amd.qmaps import QValueMaps

ap = argparse.ArgumentParser()
ap.add_argument("variables", nargs="*", help="variables/ directories of saved models (default: the two shipped policies)")
ap.add_argument("--goal", type=float, nargs=2, default=[50, 50], help="the goal in world units (the reference: 50 50)")
ap.add_argument("--world", type=int, default=100, help="cells per side (the reference: 100)")
ap.add_argument("--sectors", type=int, default=8, help="headings (the reference: 8)")
ap.add_argument("--out", default="qvalue_maps", help="directory of the PNGs (or the .npy files)")
args = ap.parse_args()

if args.variables:
    names = [os.path.basename(os.path.dirname(os.path.abspath(d).rstrip(os.sep))) or "model%d" % i for i, d in enumerate(args.variables)]
    bank = QNetworkBank.from_saved_model(args.variables, 1)
else:
    z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_policies.npz"))
    names = ["no_obs", "with_obs"]
    bank = QNetworkBank([[(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)] for tag in names], 1)

maps = QValueMaps.reference(bank, args.world, args.sectors)
action, value = maps.maps([args.goal])                          # [P, 1, S, H, W] each
action, value = action[:, 0].cpu().numpy(), value[:, 0].cpu().numpy()

COLOURS = np.array([[68, 1, 84], [33, 145, 140], [253, 231, 37]], dtype=np.uint8)     # turn left, turn right, straight
os.makedirs(args.out, exist_ok=True)
try:
    from PIL import Image
except ImportError:
    Image = None
written = 0
for p, name in enumerate(names):
    lo, hi = float(value[p].min()), float(value[p].max())
    print("%s: Q in [%.4g, %.4g]; actions %s" % (name, lo, hi, np.bincount(action[p].reshape(-1), minlength=3).tolist()))
    for k in range(args.sectors):
        grey = np.round(255.0 * (value[p, k] - lo) / max(hi - lo, 1e-30)).astype(np.uint8)
        # imshow(origin="lower"): row 0 at the bottom; a white column between the two images
        both = np.concatenate([np.repeat(grey[::-1, :, None], 3, axis=2), np.full((args.world, 4, 3), 255, dtype=np.uint8),
                               COLOURS[action[p, k]][::-1]], axis=1)
        stem = os.path.join(args.out, "%02d_%s_sector_%d_angle_%+04d" % (p, name, k, round(360 * k / args.sectors - 180)))
        if Image is not None:
            Image.fromarray(both, "RGB").save(stem + ".png")
        else:
            np.save(stem + ".npy", both)
        written += 1
print("wrote %d %s to %s" % (written, "PNGs" if Image is not None else ".npy files", args.out))
