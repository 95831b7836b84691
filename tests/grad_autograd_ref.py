"""Expected gradients of orth_project from torch.autograd in float64: no hand-written derivative.

The reference's chain splits into two parts:

* decisions that are not differentiable -- every pixel's cell and validity, and the winning pixel
  of each max / min cell -- are taken from the CPU oracle (``oracle.orth_project(..., debug=True)``),
  whose float32 cells are bit-identical with the kernels'.  A cell's winner follows torch_scatter's
  CPU rule: visiting the pixels in index order, a value replaces the cell's only when strictly
  greater (max) / smaller (min), so the winner is the lowest index whose value equals the result,
  and there is none where the result is still the cell's initial value (mask unset).
* the values are restated in torch and differentiated by autograd: the heights
  y2 = (Ry^T (Rp^T (ray_x z, ray_y z, z) + (0, h, 0)) + t)[1] with both rotations built as the
  reference builds them (I + sin(a) S + (1 - cos(a)) S^2, |a| <= 1e-3 clamped to 0, the clamp
  decided on the float32 angle), in float64; the value maps in their own dtype, so value
  gradients come out exactly as autograd forms them in float32 (the gathered weight, or
  weight / count for mean).  Both are gathered / index_add-ed into the oracle's cells.

The loss is sum(W_top * topdown) + sum(W_height * height_map); ``reference_grads`` returns its
gradients with respect to depth, value, cam_pitch and cam_height, each in the shape it was given
(a cam_height with one row for B frames gets the sum over the frames).
"""
import numpy as np
import torch

_F64 = torch.float64
_S_X = ((0., 0., 0.), (0., 0., -1.), (0., 1., 0.))     # cross-product matrix of the X axis (pitch)
_S_Y = ((0., 0., 1.), (0., 0., 0.), (-1., 0., 0.))     # of the Y axis (yaw)


def _rotation(angle, axis_s):
  """(B, 3, 3) float64 rotation about a unit axis, in the reference's form; angle (B,) float64."""
  s_mat = torch.tensor(axis_s, dtype=_F64)
  s2 = s_mat @ s_mat
  live = torch.abs(angle.detach().to(torch.float32)) > 0.001
  a = torch.where(live, angle, torch.zeros_like(angle))
  a = a.view(-1, 1, 1)
  return torch.eye(3, dtype=_F64) + torch.sin(a) * s_mat + (1 - torch.cos(a)) * s2


def _rays(H, W, cx, cy, fx, fy, flip_h):
  """float32 image-plane rays (ray_x, ray_y) of the N = H*W pixels, as float64 (N,)."""
  rows = np.arange(H, dtype=np.float32)
  if flip_h:
    rows = np.float32(H - 1) - rows
  ay = np.repeat((rows - np.float32(cy)) / np.float32(fy), W)
  ax = np.tile((np.arange(W, dtype=np.float32) - np.float32(cx)) / np.float32(fx), H)
  return torch.from_numpy(ax.astype(np.float64)), torch.from_numpy(ay.astype(np.float64))


def heights(depth, pitch, cam_height, fixed):
  """y2 (B, dc, N) float64 from depth (B, dc, N) float64 and per-frame pitch / cam_height (B,)."""
  ax, ay = fixed["rays"]
  z = torch.where(fixed["ok"], depth, torch.zeros_like(depth))     # invalid pixels stay out of the graph
  pts = torch.stack((ax * z, ay * z, z), dim=-1)                    # camera space (B, dc, N, 3)
  zeros = torch.zeros_like(cam_height)
  pts = torch.einsum("bji,bcnj->bcni", _rotation(pitch, _S_X), pts)
  pts = pts + torch.stack((zeros, cam_height, zeros), -1).view(-1, 1, 1, 3)
  if fixed["to_global"]:
    pose = fixed["pose"]
    pts = torch.einsum("bji,bcnj->bcni", _rotation(pose[:, 2], _S_Y), pts)
    pts = pts + torch.stack((pose[:, 0], torch.zeros_like(pose[:, 0]), pose[:, 1]), -1).view(-1, 1, 1, 3)
  return pts[..., 1]


def _reduce(vals, plan, reduction, size):
  """Differentiable scatter of vals (flattened) into ``size`` cells with the fixed plan."""
  out = torch.zeros(size, dtype=vals.dtype)
  if reduction in ("max", "min"):
    return out.index_put((plan["win_cell"],), vals[plan["win_pix"]])
  out = out.index_add(0, plan["cell"], vals[plan["pix"]])
  if reduction == "mean":
    out = out / plan["count"].to(vals.dtype)
  return out


def chain(fixed, depth, value, pitch, cam_height):
  """(topdown (B, oc, M), height map (B, dc, M) or None): the differentiable part of the chain with
  the cells and winners of ``fixed`` (``prepare``).  depth, pitch, cam_height float64 of shapes
  (B, dc, N), (B,), (B,); value (B, vc, N) in any float dtype, or None."""
  B, dc, oc, M = fixed["B"], fixed["dc"], fixed["oc"], fixed["M"]
  y2 = heights(depth, pitch, cam_height, fixed)
  if fixed["vc"]:
    top = _reduce(value.reshape(-1), fixed["top"], fixed["reduction"], B * oc * M)
  else:
    top = _reduce(y2.reshape(-1), fixed["top"], fixed["reduction"], B * oc * M)
  hmap = None
  if fixed["height"] is not None:
    hmap = _reduce(y2.reshape(-1), fixed["height"], "max", B * dc * M).view(B, dc, M)
  return top.view(B, oc, M), hmap


def _plan(cell, ok, vals, res, mask, oc, dc, M, reduction):
  """Fixed scatter plan for oc output channels; channel k reads the cells of depth channel
  (0 if dc == 1 else k).  cell / ok (B, dc, N); vals (B, oc, N) float32 or None (sum / mean);
  res / mask (B, oc, M) the forward's result and changed-mask (max / min)."""
  B, _, N = cell.shape
  k_dc = np.zeros(oc, dtype=np.int64) if dc == 1 else np.arange(oc)
  c = cell[:, k_dc]                                                   # (B, oc, N)
  o = ok[:, k_dc]
  base = (np.arange(B)[:, None, None] * oc + np.arange(oc)[None, :, None]) * M
  flat_cell = base + c                                                # index into (B, oc, M)
  flat_pix = (np.arange(B)[:, None, None] * oc + np.arange(oc)[None, :, None]) * N + np.arange(N)
  if reduction in ("max", "min"):
    flat_res = res.reshape(-1)
    cand = o.copy()
    cand[o] = (vals[o] == flat_res[flat_cell[o]]) & mask.reshape(-1)[flat_cell[o]]
    win = np.full(B * oc * M, N, dtype=np.int64)
    np.minimum.at(win, flat_cell[cand], np.broadcast_to(np.arange(N), cand.shape)[cand])
    has = np.nonzero(win < N)[0]
    win_pix = (has // M) * N + win[has]                               # (b, k) row of the cell, its winner
    return {"win_cell": torch.from_numpy(has), "win_pix": torch.from_numpy(win_pix)}
  count = np.bincount(flat_cell[o], minlength=B * oc * M)
  return {"cell": torch.from_numpy(flat_cell[o]), "pix": torch.from_numpy(flat_pix[o]),
          "count": torch.from_numpy(np.maximum(count, 1).astype(np.float32))}


def _oracle_cells(depth, kw, value, valid):
  from oracle import oracle
  okw = {k: v for k, v in kw.items() if k != "get_height_map"}
  okw["cam_pitch"] = np.asarray(kw["cam_pitch"], np.float32).reshape(-1)
  okw["cam_height"] = np.asarray(kw["cam_height"], np.float32).reshape(-1)
  return oracle.orth_project(depth, value_map=value, valid_map=valid, get_height_map=value is not None,
                             debug=True, nthreads=8, **okw)


def prepare(depth, kw, value=None, valid=None, cells_from=None, need_height=True):
  """The non-differentiable decisions of one orth_project call (keyword arguments ``kw``).
  ``cells_from``: the oracle's ``orth_project(..., debug=True)`` result for these inputs
  (topdown, mask[, height], debug dict), with the height map when there is a value map;
  computed here when None."""
  depth = np.asarray(depth, np.float32)
  B, dc, H, W = depth.shape
  vc = 0 if value is None else value.shape[1]
  oc = vc or dc
  mh, mw = int(kw["map_height"]), int(kw["map_width"])
  M = mh * mw
  res = cells_from if cells_from is not None else _oracle_cells(depth, kw, value, valid)
  dbg = res[-1]
  xb, zb = dbg["x_bin"], dbg["z_bin"]
  ok = dbg["valid"] & (xb >= 0) & (xb < mw) & (zb >= 0) & (zb < mh)
  cell = np.where(ok, zb * mw + xb, 0)
  red = kw.get("reduction") or "max"
  red = getattr(red, "value", red)
  vals = value.reshape(B, vc, -1).astype(np.float32) if vc else dbg["y"]
  fixed = {"B": B, "dc": dc, "vc": vc, "oc": oc, "M": M, "reduction": red,
           "ok": torch.from_numpy(ok),
           "rays": _rays(H, W, kw["center_x"], kw["center_y"], kw["focal_x"], kw["focal_y"], kw["flip_h"]),
           "to_global": bool(kw["to_global"]),
           "pose": torch.from_numpy(np.broadcast_to(np.asarray(kw["cam_pose"], np.float32).reshape(-1, 3),
                                                    (B, 3)).astype(np.float64)),
           "top": _plan(cell, ok, vals if red in ("max", "min") else None,
                        res[0], res[1], oc, dc, M, red),
           "height": None}
  if vc and need_height:
    hres = np.ascontiguousarray(res[2][:, :dc] if dc > 1 else res[2][:, :1])
    fixed["height"] = _plan(cell, ok, dbg["y"], hres, hres != -np.inf, dc, dc, M, "max")
  return fixed


def _leaf(x, dtype):
  return torch.as_tensor(np.asarray(x), dtype=dtype).clone().requires_grad_()


def reference_grads(depth, kw, *, W_top, W_height=None, value=None, valid=None, cells_from=None):
  """d loss / d (depth, value, cam_pitch, cam_height) for loss = sum(W_top * topdown)
  + sum(W_height * height_map), the height map broadcast over the value channels as
  orth_project returns it (without a value map it is topdown itself).

  depth (B, dc, H, W), value (B, vc, H, W) or None, valid as orth_project takes it (numpy);
  kw: orth_project's keyword arguments, cam_pitch / cam_height with 1 or B elements in any shape.
  Returns a dict: grad_depth float64, grad_value in the value's dtype (float32 unless given
  otherwise), grad_pitch / grad_cam_height float64 in the shapes of cam_pitch / cam_height."""
  depth = np.asarray(depth)
  B = depth.shape[0]
  fixed = prepare(depth.astype(np.float32), kw, value=None if value is None else np.asarray(value, np.float32),
                  valid=valid, cells_from=cells_from, need_height=W_height is not None)
  d = _leaf(depth.astype(np.float32), _F64)
  v = None if value is None else _leaf(value, torch.as_tensor(np.asarray(value)).dtype)
  p = _leaf(np.asarray(kw["cam_pitch"], np.float32), _F64)
  h = _leaf(np.asarray(kw["cam_height"], np.float32), _F64)
  per_frame = lambda t: t.reshape(-1).expand(B) if t.numel() == 1 else t.reshape(-1)
  top, hmap = chain(fixed, d.reshape(B, fixed["dc"], -1), None if v is None else v.reshape(B, fixed["vc"], -1),
                    per_frame(p), per_frame(h))
  wt = torch.as_tensor(np.asarray(W_top)).reshape(top.shape)
  loss = (wt.to(top.dtype) * top).sum().to(_F64)
  if W_height is not None:
    wh = torch.as_tensor(np.asarray(W_height)).reshape(top.shape).to(_F64)
    if hmap is None:
      loss = loss + (wh * top.to(_F64)).sum()
    else:
      loss = loss + (wh * torch.broadcast_to(hmap, top.shape)).sum()
  inputs = [x for x in (d, v, p, h) if x is not None]
  grads = torch.autograd.grad(loss, inputs, allow_unused=True)
  grads = [torch.zeros_like(x) if g is None else g for x, g in zip(inputs, grads)]
  out = dict(zip(["grad_depth"] + (["grad_value"] if v is not None else []) + ["grad_pitch", "grad_cam_height"],
                 [g.detach().numpy() for g in grads]))
  return out
