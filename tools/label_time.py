#!/usr/bin/env python3
"""Event timing of the label route of orth_project against the one-hot route, in one process, alternating.

Workloads (bench.py's geometry, max reduction, fill 0, to_global):
  cfg3  B=64, 640x480, 40 classes -> 512x512 object maps
  demo  B=1,  800x600,  5 classes -> 600x600 (the reference's object-map demo)
Per repeat, each timed as the median of --iters calls between device events, inputs rotated over sets
that each exceed the Infinity Cache where the workload's inputs do:
  (a) one_hot        the existing call, value map prepared outside the timed window (the yardstick)
  (b) labels_uint8 / labels_int64   the label call (and, with --policies, its expansion's stores forced
                     non-temporal / default: dm_debug_force_nt_fill)
  (c) end_to_end     one_hot + permute + float + (a), as a caller of the value-map door pays it
The spread of (a) against itself over the repeats is printed with the result, and the byte model of
both routes computed from the shapes: call time by events, bytes by model.

Usage:  python tools/label_time.py [--iters 10] [--repeats 3] [--workloads cfg3,demo] [--height] [--policies]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dungeon_maps_amd as dmap  # noqa: E402
from dungeon_maps_amd import _native  # noqa: E402

WORKLOADS = {"cfg3": (64, 480, 640, 512, 512, 40, 0.03), "demo": (1, 600, 800, 600, 600, 5, 0.015)}
INFINITY_CACHE = 256 << 20


def timed(fn, sets, iters):
  for s in sets:                       # warm-up on every set
    fn(s)
  ts = []
  for i in range(iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn(sets[i % len(sets)])
    b.record()
    b.synchronize()
    del out
    ts.append(a.elapsed_time(b) * 1e3)
  return float(np.median(ts))


def byte_model(B, H, W, mh, mw, C, label_bytes, height):
  n, cells = B * H * W, B * mh * mw
  maps = cells * C * 5                                     # maps (f32) and masks (u8), written once
  hmap = cells * 5 + n * 4 if height else 0                # the heights projection: depth again, map + mask
  one_hot = {"read": n * 4 + n * C * 4 + hmap // 2, "written": maps + hmap}
  labels = {"read": n * 4 + n * label_bytes + cells * 8, "class_words_zeroed": cells * 8,
            "written": maps + (cells * 5 if height else 0), "height_pass_depth_read": n * 4 if height else 0}
  return {"one_hot_route": one_hot, "label_route": labels, "maps_and_masks": maps,
          "caller_one_hot_tensor": n * C * 4, "caller_int64_intermediate": n * C * 8}


def run(name, iters, repeats, height, policies):
  B, H, W, mh, mw, C, res = WORKLOADS[name]
  g = torch.Generator(device="cuda").manual_seed(1)
  rng = np.random.default_rng(0)
  proj = dmap.MapProjector(width=W, height=H, hfov=np.radians(70.), cam_pitch=np.radians(-20.), cam_height=0.88,
                           width_offset=mw / 2., height_offset=mh / 2., map_res=res, map_width=mw,
                           map_height=mh, trunc_depth_min=0.15, trunc_depth_max=5.05, to_global=True,
                           fill_value=0.0)
  pose = torch.tensor(np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-3, 3, B)], 1),
                      dtype=torch.float32)
  n_sets = 2 if B * C * H * W * 4 > INFINITY_CACHE else 4
  sets = []
  for _ in range(n_sets):
    d = torch.empty(B, 1, H, W, device="cuda").uniform_(0.1, 10.0, generator=g)
    l64 = torch.randint(0, C, (B, 1, H, W), device="cuda", generator=g)
    v = torch.nn.functional.one_hot(l64[:, 0], C).permute(0, 3, 1, 2).float().contiguous()
    sets.append((d, v, l64.to(torch.uint8), l64))
  kw = dict(cam_pose=pose, get_height_map=height)
  lib = _native.lib()
  one_hot = lambda s: proj.orth_project(s[0], value_map=s[1], **kw)
  lab8 = lambda s: proj.orth_project(s[0], label_map=s[2], num_classes=C, **kw)
  lab64 = lambda s: proj.orth_project(s[0], label_map=s[3], num_classes=C, **kw)
  e2e = lambda s: proj.orth_project(
      s[0], value_map=torch.nn.functional.one_hot(s[3][:, 0], C).permute(0, 3, 1, 2).float().contiguous(), **kw)
  # same results, and the native route
  want, got = one_hot(sets[0]), lab8(sets[0])
  assert lib.dm_debug_last_label_route() == _native.LABEL_ROUTE_NATIVE
  assert all(torch.equal(a, b) for a, b in zip(want, got)), "label call differs from the one-hot call"
  del want, got
  rows = {"one_hot": [], "labels_uint8": [], "labels_int64": [], "end_to_end": []}
  if policies:
    rows.update({"labels_uint8_nt": [], "labels_uint8_default_policy": []})
  for _ in range(repeats):
    rows["one_hot"].append(timed(one_hot, sets, iters))
    rows["labels_uint8"].append(timed(lab8, sets, iters))
    rows["labels_int64"].append(timed(lab64, sets, iters))
    rows["end_to_end"].append(timed(e2e, sets, iters))
    if policies:
      for key, mode in (("labels_uint8_nt", 1), ("labels_uint8_default_policy", 0)):
        lib.dm_debug_force_nt_fill(mode)
        try:
          rows[key].append(timed(lab8, sets, iters))
        finally:
          lib.dm_debug_force_nt_fill(-1)
  a = rows["one_hot"]
  spread = max(a) - min(a)
  med = {k: float(np.median(v)) for k, v in rows.items()}
  print(json.dumps({
      "workload": name, "B": B, "image": f"{W}x{H}", "map": f"{mw}x{mh}", "classes": C, "height_map": height,
      "what": "call time by device events, us: median of --iters calls per repeat, all repeats listed",
      "us": {k: [round(t, 1) for t in v] for k, v in rows.items()},
      "median_us": {k: round(t, 1) for k, t in med.items()},
      "one_hot_spread_us": round(spread, 1),
      "labels_uint8_faster_than_one_hot_by_us": round(med["one_hot"] - med["labels_uint8"], 1),
      "condition_met": bool(max(rows["labels_uint8"]) + spread < min(a)),
      "bytes_by_model": byte_model(B, H, W, mh, mw, C, 1, height)}), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--repeats", type=int, default=3)
  ap.add_argument("--workloads", default="cfg3,demo")
  ap.add_argument("--height", action="store_true", help="with get_height_map=True (what MapBuilder.plot asks for)")
  ap.add_argument("--policies", action="store_true", help="also time the expansion with both store policies")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit("label_time.py measures on a GPU; none is visible")
  for name in args.workloads.split(","):
    run(name, args.iters, args.repeats, args.height, args.policies)


if __name__ == "__main__":
  main()
