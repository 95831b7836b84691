#!/usr/bin/env python3
"""Generate g14: gradients of the REFERENCE's own orth_project (autograd on CPU, float32).

Runs only in the build container, next to gen_golden.py, whose conventions it follows: the
reference's ``maps.py`` / ``utils.py`` run unmodified, B = 1 per call, batched cases are a stack
of B = 1 results.  The third-party ``torch-scatter`` (absent from the image) is restated here
WITH its backward, because the forward-only restatement of gen_golden.py differentiates through
``scatter_reduce_``, whose backward splits ties -- not what torch-scatter does:

* max / min: a custom autograd.Function.  Forward as torch-scatter's CPU kernel: the existing
  ``out`` values take part, a source element replaces the cell's value only when strictly
  greater (max) / smaller (min), visited in index order; NaN never wins.  The arg of a cell is
  therefore the LOWEST source index whose value equals the result, provided the result differs
  from the cell's initial value (else no arg).  Backward: the cell's gradient goes to its arg
  only (torch-scatter scatters grad_out at arg_out and drops the "no arg" slot).
* sum: ``out.scatter_add_`` -- torch's own backward is torch-scatter's (a gather).
* mean: ``scatter_add_`` then ``true_divide_(count)`` -- backward gather / count, as torch-scatter.

Loss per case: sum(W * topdown) (+ sum(Wh * height_map) with get_height_map and a value map)
for fixed random weights; saved: the gradients with respect to depth, value, cam_pitch and
cam_height, with the inputs, weights, the forward outputs and the configuration.  The .npz is
written with fixed zip timestamps, so a rerun reproduces it byte for byte.

g15 (CASES_G15) covers what g14's cases leave out, with per-case options: a loss on the height map
alone (no topdown term: ``loss_top`` is saved as 0), one 0-d cam_height shared by both frames (the
frames' gradients summed, saved 0-d) and pitches set exactly in float32 (the |a| <= 1e-3 clamp's
edge).

Usage:  python tests/golden/gen_golden_grad.py
        (writes tests/golden/g14_orth_project_grad.npz and tests/golden/g15_orth_project_grad.npz)
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (scene_depth, T, the reference's location)

NAME = "g14_orth_project_grad"
NAME_G15 = "g15_orth_project_grad"


class _ScatterArg(torch.autograd.Function):
  """torch-scatter's scatter_max / scatter_min into ``out`` (in place), arg-based backward."""

  @staticmethod
  def forward(ctx, src, index, out, is_max):
    index = index.expand_as(src) if index.shape != src.shape else index
    n = src.shape[-1]
    rows_src = src.reshape(-1, n)
    rows_idx = index.reshape(-1, n)
    rows_out = out.view(-1, out.shape[-1])
    init = rows_out.clone()
    bad = np.inf * (-1 if is_max else 1)
    s = torch.where(torch.isnan(rows_src), torch.full_like(rows_src, bad), rows_src)
    rows_out.scatter_reduce_(-1, rows_idx, s, reduce="amax" if is_max else "amin", include_self=True)
    res = rows_out.gather(-1, rows_idx)
    cand = (s == res) & (res != init.gather(-1, rows_idx))
    pos = torch.arange(n).expand_as(rows_idx)
    arg = torch.full_like(rows_out, n, dtype=torch.int64)
    arg.scatter_reduce_(-1, rows_idx, torch.where(cand, pos, torch.full_like(pos, n)),
                        reduce="amin", include_self=True)
    ctx.mark_dirty(out)
    ctx.save_for_backward(arg)
    ctx.shape = src.shape
    return out

  @staticmethod
  def backward(ctx, grad_out):
    (arg,) = ctx.saved_tensors
    n = ctx.shape[-1]
    g = grad_out.reshape(arg.shape)
    grad_src = torch.zeros((arg.shape[0], n + 1), dtype=g.dtype)
    grad_src.scatter_(-1, arg, g)            # cells without an arg land in the dropped slot n
    return grad_src[:, :n].reshape(ctx.shape), None, None, None


def _install_torch_scatter():
  mod = types.ModuleType("torch_scatter")

  def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    assert out is not None and dim == -1
    return _ScatterArg.apply(src, index, out, True), None

  def scatter_min(src, index, dim=-1, out=None, dim_size=None):
    assert out is not None and dim == -1
    return _ScatterArg.apply(src, index, out, False), None

  def _expand(index, src):
    return index.expand_as(src) if index.shape != src.shape else index

  def scatter_add(src, index, dim=-1, out=None, dim_size=None):
    out.scatter_add_(dim, _expand(index, src), src)
    return out

  def scatter_mean(src, index, dim=-1, out=None, dim_size=None):
    index = _expand(index, src)
    out.scatter_add_(dim, index, src)
    count = torch.zeros_like(out)
    count.scatter_add_(dim, index, torch.ones_like(src))
    count[count < 1] = 1
    out.true_divide_(count)
    return out

  def scatter_mul(src, index, dim=-1, out=None, dim_size=None):
    raise NotImplementedError("prod has no backward here")

  mod.scatter_max, mod.scatter_min = scatter_max, scatter_min
  mod.scatter_add, mod.scatter_mean, mod.scatter_mul = scatter_add, scatter_mean, scatter_mul
  sys.modules["torch_scatter"] = mod


def _import_reference():
  _install_torch_scatter()
  sys.path.insert(0, gg.REFERENCE)
  import dungeon_maps as dmap  # noqa: E402
  assert dmap.__version__ == "0.0.3a1", dmap.__version__
  return dmap


H, W = 48, 64
HFOV = np.radians(70.)
BASE = dict(width=W, height=H, hfov=HFOV, width_offset=16., height_offset=16., map_res=0.2,
            map_width=32, map_height=32)

# name, reduction, fill, value ('none' / 'onehot' / 'cont'), value channels, depth channels,
# valid map, clip_border, (dmin, dmax, hmax), to_global, flip_h, get_height_map, pitches (one per frame)
CASES = [
    ("max_height", "max", -np.inf, "none", 0, 1, False, None, (0.15, 5.05, 1.2), True, True, False, (-20., -15.)),
    ("min_height", "min", None, "none", 0, 1, True, 2, (0.15, None, None), True, True, False, (-20., 0.03)),
    ("sum_height", "sum", None, "none", 0, 1, False, 3, (None, 5.05, None), False, True, False, (-20., -25.)),
    ("mean_height", "mean", 2.0, "none", 0, 1, True, None, (0.15, 5.05, 1.2), True, False, False, (-18., -20.)),
    ("max_onehot", "max", None, "onehot", 5, 1, True, None, (0.15, 5.05, None), False, False, True, (-20., -22.)),
    ("max_cont", "max", -np.inf, "cont", 3, 3, False, 2, (None, 5.05, 1.2), True, True, True, (-20., -10.)),
    ("min_cont", "min", np.inf, "cont", 2, 1, False, None, (0.15, 5.05, None), True, True, True, (-20., -25.)),
    ("sum_onehot", "sum", None, "onehot", 4, 1, True, 2, (0.15, None, None), True, False, True, (-20., -20.)),
    ("mean_cont", "mean", None, "cont", 3, 3, True, None, (0.15, 5.05, 1.2), True, True, True, (-20., -15.)),
    ("max_pitch_clamp", "max", None, "none", 0, 1, False, None, (0.15, 5.05, None), True, True, False,
     (float(np.degrees(0.0005)), -20.)),
]
_EPS32 = np.float32(0.001)
# as CASES, plus options: loss_top (False: the loss has no topdown term), shared_height (one 0-d
# cam_height for both frames), pitch (float32 radians, replacing the pitches' values; the scenes
# still use the pitches in degrees)
CASES_G15 = [
    ("max_height_dc3", "max", -np.inf, "none", 0, 3, True, None, (0.15, 5.05, None), True, True, False,
     (-20., -15.), {}),
    ("min_cont_local_height", "min", None, "cont", 3, 1, True, None, (0.15, 5.05, None), False, True, True,
     (-20., -25.), {}),
    ("max_height_fill_in_range", "max", 0.002, "none", 0, 1, False, None, (0.15, 5.05, None), True, True, False,
     (-20., -18.), {}),
    ("height_only_loss_onehot", "max", None, "onehot", 4, 1, True, None, (0.15, 5.05, None), True, True, True,
     (-20., -22.), {"loss_top": False}),
    ("max_onehot_shared_cam_height", "max", None, "onehot", 3, 1, False, None, (0.15, 5.05, None), True, False,
     True, (-20., -20.), {"shared_height": True}),
    ("max_pitch_at_eps", "max", None, "none", 0, 1, False, None, (0.15, 5.05, None), True, True, False,
     (float(np.degrees(0.001)), float(np.degrees(0.001))),
     {"pitch": np.array([_EPS32, np.nextafter(_EPS32, np.float32(1))], dtype=np.float32)}),
]
POSES = np.array([[0.2, 0.1, -0.3], [-0.4, 0.3, 0.7]], dtype=np.float32)
CAM_H = np.array([0.88, 1.05], dtype=np.float32)


def _case_inputs(rng, vkind, vc, dc, use_valid, pitches):
  B = len(pitches)
  depth = np.stack([np.stack([gg.scene_depth(rng, H, W, HFOV, np.radians(p), CAM_H[b])
                              for _ in range(dc)]) for b, p in enumerate(pitches)])
  value = None
  if vkind == "onehot":
    cls = rng.integers(0, vc, size=(B, 1, H, W))
    cls[:, :, :, : W // 2] = 1                    # a large block of one class: ties in every cell
    value = (np.arange(vc)[None, :, None, None] == cls).astype(np.float32)
  elif vkind == "cont":
    value = rng.uniform(0.0, 2.0, size=(B, vc, H, W)).astype(np.float32)
  valid = (rng.uniform(size=(B, dc, H, W)) > 0.2) if use_valid else None
  return depth.astype(np.float32), value, valid


def run_case(dmap, rng, case):
  (name, red, fill, vkind, vc, dc, use_valid, clip, (dmin, dmax, hmax), to_global, flip_h,
   get_height, pitches) = case[:13]
  opts = case[13] if len(case) > 13 else None
  depth, value, valid = _case_inputs(rng, vkind, vc, dc, use_valid, pitches)
  B = depth.shape[0]
  oc = vc if vc else dc
  weights = rng.normal(size=(B, oc, 32, 32)).astype(np.float32)
  hweights = rng.normal(size=(B, oc, 32, 32)).astype(np.float32)
  pitch = np.radians(np.asarray(pitches, dtype=np.float64)).astype(np.float32)
  loss_top, shared_h, cam_h = True, False, CAM_H[:B].copy()
  if opts is not None:
    loss_top, shared_h = opts.get("loss_top", True), opts.get("shared_height", False)
    pitch = opts.get("pitch", pitch)
    if shared_h:
      cam_h = np.full(B, CAM_H[0], dtype=np.float32)
  out = {f"{name}/depth": depth, f"{name}/weights": weights, f"{name}/pitch": pitch,
         f"{name}/cam_height": cam_h[0].copy() if shared_h else cam_h, f"{name}/cam_pose": POSES[:B].copy()}
  if opts is not None:
    out[f"{name}/loss_top"] = np.asarray(int(loss_top))
  if value is not None:
    out[f"{name}/value"] = value
  if valid is not None:
    out[f"{name}/valid"] = valid
  if get_height and vc:
    out[f"{name}/hweights"] = hweights
  grads = {k: [] for k in ("topdown", "mask", "grad_depth", "grad_value", "grad_pitch", "grad_cam_height")}
  for b in range(B):
    proj = dmap.MapProjector(**BASE, cam_pitch=0.0, cam_height=0.0, trunc_depth_min=dmin,
                             trunc_depth_max=dmax, trunc_height_max=hmax, clip_border=clip,
                             to_global=to_global, flip_h=flip_h, fill_value=fill, reduction=red)
    d = torch.tensor(depth[b:b + 1]).requires_grad_()
    v = None if value is None else torch.tensor(value[b:b + 1]).requires_grad_()
    m = None if valid is None else torch.tensor(valid[b:b + 1])
    p = torch.tensor(pitch[b:b + 1]).requires_grad_()
    h = torch.tensor(cam_h[b:b + 1]).requires_grad_()
    outs = proj.orth_project(depth_map=d, value_map=v, valid_map=m, cam_pose=torch.tensor(POSES[b:b + 1]),
                             cam_pitch=p, cam_height=h, get_height_map=get_height)
    loss = (torch.tensor(weights[b:b + 1]) * outs[0]).sum() if loss_top else 0
    if get_height and vc:
      loss = loss + (torch.tensor(hweights[b:b + 1]) * outs[2]).sum()
    loss.backward()
    grads["topdown"].append(outs[0].detach().numpy())
    grads["mask"].append(outs[1].numpy())
    grads["grad_depth"].append(d.grad.numpy())
    if v is not None:
      grads["grad_value"].append(np.zeros_like(value[b:b + 1]) if v.grad is None else v.grad.numpy())
    grads["grad_pitch"].append(p.grad.numpy())
    grads["grad_cam_height"].append(h.grad.numpy())
  for k, lst in grads.items():
    if lst:
      out[f"{name}/{k}"] = np.concatenate(lst)
  if shared_h:                                     # one cam_height for both frames: the frames' sum
    out[f"{name}/grad_cam_height"] = out[f"{name}/grad_cam_height"].sum(dtype=np.float32)
  cfg = dict(reduction=red, fill=np.nan if fill is None else fill, fill_is_none=fill is None,
             dmin=np.nan if dmin is None else dmin, dmax=np.nan if dmax is None else dmax,
             hmax=np.nan if hmax is None else hmax, clip=0 if clip is None else clip,
             to_global=to_global, flip_h=flip_h, get_height=get_height)
  for k, val in cfg.items():
    out[f"{name}/cfg_{k}"] = np.asarray(val)
  return out


def save_reproducible(path, arrays):
  """np.savez layout (one .npy per key) with fixed zip timestamps and order."""
  with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
    for key in sorted(arrays):
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
      info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      zf.writestr(info, buf.getvalue())
  print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KiB")


def main():
  torch.set_num_threads(1)
  torch.manual_seed(0)
  dmap = _import_reference()
  for name, cases, seed in ((NAME, CASES, 1414), (NAME_G15, CASES_G15, 1515)):
    rng = np.random.default_rng(seed)
    arrays = {"cases": np.array([c[0] for c in cases]),
              **{f"cfg_{k}": np.asarray(v) for k, v in BASE.items()}}
    for case in cases:
      arrays.update(run_case(dmap, rng, case))
    save_reproducible(os.path.join(HERE, name + ".npz"), arrays)


if __name__ == "__main__":
  main()
