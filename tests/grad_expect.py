"""Expected gradients of orth_project in numpy, from the CPU oracle's per-pixel intermediates.

``oracle.orth_project(..., debug=True)`` gives every pixel's bins (x_bin, z_bin), validity and
height y.  From them and the forward outputs this module restates the reference's chain rule
(tests/golden/gen_golden_grad.py produces the reference's own numbers, g14):

* max / min: a cell's gradient goes to its winner, the lowest flat pixel index whose value equals
  the cell's result, when the cell's mask is set; sum: to every pixel; mean: divided by the
  cell's count of valid in-bounds pixels.
* heights: y2 = Ry_row1 . (Rp^T (X, Y, z) + (0, h, 0)), X = ray_x z, Y = ray_y z; Ry's row 1 is
  (0, 1, 0) for a rotation about Y, so dy2/dz = ray_x Rp[1] + ray_y Rp[4] + Rp[7],
  dy2/dh = 1 and dy2/dpitch = -sin(a) Y + cos(a) z (0 when |a| <= 1e-3).

Value gradients come out in float32 exactly as autograd forms them; the depth and camera
gradients in float64.
"""
import numpy as np

_EPS = np.float32(0.001)


def _winners(cell, ok, val, res, mask, M):
  """Lowest pixel index per cell with val == res[cell] and mask[cell]; -1 where none."""
  n = cell.shape[0]
  idx = np.arange(n)
  cand = ok.copy()
  cand[ok] = (val[ok] == res[cell[ok]]) & mask[cell[ok]]
  win = np.full(M, n, dtype=np.int64)
  np.minimum.at(win, cell[cand], idx[cand])
  win[win == n] = -1
  return win


def expected_grads(dbg, depth, topdown, mask, *, W_top, W_height=None, value=None, reduction="max",
                   pitch, H, W, cx, cy, fx, fy, flip_h, mh, mw):
  """(grad_depth (B, dc, H, W) f64, grad_value (B, vc, H, W) f32 or None,
  grad_pitch (B,) f64, grad_cam_height (B,) f64).

  dbg: the oracle's debug dict; depth (B, dc, H, W); topdown / mask: the forward outputs (B, oc, mh, mw);
  W_top: d loss / d topdown; W_height: d loss / d height map (B, oc, mh, mw) or None."""
  xb, zb, valid, y = dbg["x_bin"], dbg["z_bin"], dbg["valid"], dbg["y"]
  B, dc, N = xb.shape
  M = mh * mw
  vc = 0 if value is None else value.shape[1]
  ok = valid & (xb >= 0) & (xb < mw) & (zb >= 0) & (zb < mh)
  cell = np.where(ok, zb * mw + xb, 0)
  rows = np.arange(H, dtype=np.float32)
  if flip_h:
    rows = np.float32(H - 1) - rows
  ay = np.repeat((rows - np.float32(cy)) / np.float32(fy), W).astype(np.float64)
  ax = np.tile((np.arange(W, dtype=np.float32) - np.float32(cx)) / np.float32(fx), H).astype(np.float64)
  p32 = np.asarray(pitch, dtype=np.float32).reshape(-1)
  live = np.abs(p32) > _EPS
  a = np.where(live, p32, np.float32(0)).astype(np.float64)
  s, c = np.sin(a), np.cos(a)
  d = 1 - (1 - c)
  top = topdown.reshape(B, -1, M)
  msk = mask.reshape(B, -1, M)
  gt = W_top.reshape(B, -1, M).astype(np.float32)
  g_value = None if value is None else np.zeros((B, vc, N), dtype=np.float32)
  w = np.zeros((B, dc, N), dtype=np.float64)
  for b in range(B):
    for ch in range(dc):
      o, cl = ok[b, ch], cell[b, ch]
      count = np.bincount(cl[o], minlength=M).astype(np.float32)
      chans = range(vc) if (vc and dc == 1) else [ch]
      for k in chans:
        val = value[b, k].reshape(-1) if vc else y[b, ch]
        g = gt[b, k]
        if reduction in ("max", "min"):
          win = _winners(cl, o, val, top[b, k], msk[b, k], M)
          sel = o & (win[cl] == np.arange(N))
          gp = np.where(sel, g[cl], np.float32(0))
        elif reduction == "sum":
          gp = np.where(o, g[cl], np.float32(0))
        elif reduction == "mean":
          gp = np.where(o, g[cl] / np.maximum(count[cl], np.float32(1)), np.float32(0))
        else:
          raise ValueError(reduction)
        if vc:
          g_value[b, k] = gp
        else:
          w[b, ch] = gp
      if vc and W_height is not None:
        # the (B, dc) height map broadcast over the value channels: its gradient sums them
        gh = W_height.reshape(B, -1, M)[b].astype(np.float64)
        gh = gh.sum(0) if dc == 1 else gh[ch]
        hres = np.full(M, -np.inf)
        np.maximum.at(hres, cl[o], y[b, ch][o].astype(np.float64))
        hwin = _winners(cl, o, y[b, ch].astype(np.float64), hres, hres != -np.inf, M)
        sel = o & (hwin[cl] == np.arange(N))
        w[b, ch] = np.where(sel, gh[cl], 0.0)
  z = np.where(w != 0, depth.reshape(B, dc, N), 0.0).astype(np.float64)
  Rp1, Rp4, Rp7 = 0.0, d[:, None, None], s[:, None, None]
  dydz = ax * Rp1 + ay * Rp4 + Rp7
  g_depth = (w * dydz).reshape(B, dc, H, W)
  Y = ay * z
  MY = (w * Y).sum(axis=(1, 2))
  Mz = (w * z).sum(axis=(1, 2))
  g_pitch = np.where(live, -s * MY + c * Mz, 0.0)
  g_h = w.sum(axis=(1, 2))
  if g_value is not None:
    g_value = g_value.reshape(B, vc, H, W)
  return g_depth, g_value, g_pitch, g_h
