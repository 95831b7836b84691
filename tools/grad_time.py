#!/usr/bin/env python3
"""Event timing of orth_project's autograd path: the grad-path forward and .backward().

Workloads (bench.py's geometry, max reduction, fill -inf, to_global):
  cfg1  B=1,  320x240 -> 256x256 heights
  cfg2  B=64, 640x480 -> 512x512 heights
  cfg3  B=64, 640x480 -> 512x512, a 40-channel value map + the height map
Depth, value map, cam_pitch and cam_height require grad.  Prints one JSON line per workload with the
median times (us) of the no-grad forward, the grad-path forward and the backward, and the bytes the
two backward passes must move (winners pass: depth + values + the gathered results + the winner
buffers; gradient pass: depth + winners + the gathered gradients + grad_value / grad_depth), with the
fraction of an 8 TB/s roofline that the measured backward reaches.

Usage:  python tools/grad_time.py [--iters 20] [--workloads cfg1,cfg2,cfg3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dungeon_maps_amd as dmap  # noqa: E402

WORKLOADS = {"cfg1": (1, 240, 320, 256, 256, 0), "cfg2": (64, 480, 640, 512, 512, 0),
             "cfg3": (64, 480, 640, 512, 512, 40)}
ROOF = 8.0e12


def depth_batch(B, H, W, rng):
  r = np.arange(H)[:, None]
  base = np.where(r > H * 0.45, 0.88 / np.maximum(np.sin(np.radians(20.)) + (r - H / 2) / (0.9 * W), 0.05), 6.0)
  d = np.broadcast_to(base, (B, 1, H, W)) + rng.uniform(0.0, 0.05, size=(B, 1, H, W))
  return torch.tensor(np.clip(d, 0.1, 6.0).astype(np.float32), device="cuda")


def timed(fn, iters):
  ts = []
  for _ in range(iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    ts.append(a.elapsed_time(b) * 1e3)
  return float(np.median(ts))


def run(name, iters):
  B, H, W, mh, mw, C = WORKLOADS[name]
  rng = np.random.default_rng(0)
  proj = dmap.MapProjector(width=W, height=H, hfov=np.radians(70.), cam_pitch=np.radians(-20.), cam_height=0.88,
                           width_offset=mw / 2., height_offset=mh / 2., map_res=0.03, map_width=mw,
                           map_height=mh, trunc_depth_min=0.15, trunc_depth_max=5.05, to_global=True,
                           fill_value=-np.inf)
  depth = depth_batch(B, H, W, rng).requires_grad_()
  value = None
  if C:
    value = torch.rand((B, C, H, W), device="cuda").requires_grad_()
  pose = torch.tensor(np.stack([rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), rng.uniform(-3, 3, B)], 1),
                      dtype=torch.float32)
  pitch = torch.full((B,), np.radians(-20.), device="cuda", requires_grad=True)
  cam_h = torch.full((B,), 0.88, device="cuda", requires_grad=True)
  kw = dict(value_map=value, cam_pose=pose, cam_pitch=pitch, cam_height=cam_h, get_height_map=bool(C))
  with torch.no_grad():
    fwd_plain = timed(lambda: proj.orth_project(depth, **kw), iters)
  fwd = timed(lambda: proj.orth_project(depth, **kw), iters)
  outs = proj.orth_project(depth, **kw)
  grads = [torch.randn_like(outs[0])] + ([torch.randn_like(outs[2])] if C else [])
  heads = [outs[0]] + ([outs[2]] if C else [])

  def back():
    torch.autograd.backward(heads, grads, retain_graph=True)
  bwd = timed(back, iters)
  n, cells = B * H * W, B * mh * mw
  oc = C or 1
  # winners: depth, values, the gathered results (one per value channel + the height), winner buffers
  winners = n * 4 + n * C * 4 + n * (oc + (1 if C else 0)) * 4 + cells * (oc + (1 if C else 0)) * 4
  # gradient pass: depth, winners + gathered gradients per channel, grad_value, grad_depth
  grad_pass = n * 4 + n * (oc + (1 if C else 0)) * 8 + n * C * 4 + n * 4
  moved = winners + grad_pass
  print(json.dumps({"workload": name, "B": B, "image": f"{W}x{H}", "map": f"{mw}x{mh}", "value_channels": C,
                    "forward_no_grad_us": round(fwd_plain, 1), "forward_grad_path_us": round(fwd, 1),
                    "backward_us": round(bwd, 1), "backward_over_forward": round(bwd / fwd_plain, 2),
                    "backward_min_bytes": moved, "backward_roofline_fraction": round(moved / (bwd * 1e-6) / ROOF, 3)}),
        flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--workloads", default="cfg1,cfg2,cfg3")
  args = ap.parse_args()
  for name in args.workloads.split(","):
    run(name, args.iters)


if __name__ == "__main__":
  main()
