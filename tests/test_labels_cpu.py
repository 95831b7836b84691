"""orth_project(label_map=, num_classes=) without a GPU: every refusal happens before a device is
looked for, the C entry points validate their arguments before any HIP call, and the object API
forwards the two arguments."""
import ctypes
import inspect

import numpy as np
import pytest
import torch


def _kw(**over):
  kw = dict(valid_map=None, cam_pose=np.zeros(3, np.float32), width_offset=4., height_offset=4.,
            cam_pitch=0., cam_height=1., map_res=0.5, map_width=8, map_height=8, focal_x=4., focal_y=4.,
            center_x=3.5, center_y=1.5, trunc_depth_min=None, trunc_depth_max=None,
            trunc_height_max=None, clip_border=None, to_global=False)
  kw.update(over)
  return kw


DEPTH = np.full((1, 1, 4, 8), 2.0, np.float32)
LABELS = np.zeros((1, 1, 4, 8), np.int64)


@pytest.mark.parametrize("what,args", [
    ("exclude", dict(value_map=np.zeros((1, 3, 4, 8), np.float32), label_map=LABELS, num_classes=3)),
    ("needs `num_classes`", dict(value_map=None, label_map=LABELS)),
    ("without a `label_map`", dict(value_map=None, num_classes=3)),
    ("int >= 1", dict(value_map=None, label_map=LABELS, num_classes=0)),
    ("int >= 1", dict(value_map=None, label_map=LABELS, num_classes=2.0)),
    ("int >= 1", dict(value_map=None, label_map=LABELS, num_classes=True)),
    ("uint8, int16, int32 or int64", dict(value_map=None, label_map=LABELS.astype(np.float32), num_classes=3)),
    ("uint8, int16, int32 or int64", dict(value_map=None, label_map=LABELS.astype(bool), num_classes=3)),
    ("does not match", dict(value_map=None, label_map=np.zeros((1, 1, 4, 7), np.int64), num_classes=3)),
    ("does not match", dict(value_map=None, label_map=np.zeros((2, 1, 4, 8), np.int64), num_classes=3)),
    ("does not match", dict(value_map=None, label_map=np.zeros((1, 2, 4, 8), np.int64), num_classes=3)),
])
def test_refusals_are_value_errors_raised_before_a_gpu_is_needed(what, args):
  import dungeon_maps_amd as dmap
  with pytest.raises(ValueError, match=what):
    dmap.orth_project(DEPTH, **_kw(**args))


def test_a_depth_map_of_several_channels_is_refused():
  import dungeon_maps_amd as dmap
  with pytest.raises(ValueError, match="one-channel"):
    dmap.orth_project(np.ones((1, 2, 4, 8), np.float32),
                      **_kw(value_map=None, label_map=LABELS, num_classes=3))


def test_label_layouts():
  """(b, 1, h, w) and its lower-rank forms, as the depth map; a simulator's trailing channel."""
  from dungeon_maps_amd import functional as F
  for shape in ((1, 1, 4, 8), (1, 4, 8), (4, 8), (4, 8, 1), (1, 4, 8, 1)):
    lab, code = F._label_image(np.arange(32, dtype=np.int64).reshape(shape), DEPTH, None, 3)
    assert tuple(lab.shape) == (1, 1, 4, 8) and code == 3
    np.testing.assert_array_equal(lab.numpy().ravel(), np.arange(32))
  for dt, code in ((torch.uint8, 0), (torch.int16, 1), (torch.int32, 2), (torch.int64, 3)):
    assert F._label_image(torch.zeros((4, 8), dtype=dt), DEPTH[0, 0], None, 1)[1] == code


def test_entry_points_without_labels_do_not_know_the_keyword():
  import dungeon_maps_amd as dmap
  from dungeon_maps_amd import parallel
  for fn in (dmap.orth_project_and_fuse, dmap.orth_project_fused, dmap.orth_project_and_flow,
             dmap.prepare_orth_project, parallel.project_and_fuse_sharded):
    assert "label_map" not in inspect.signature(fn).parameters, fn.__name__


def _params(**over):
  from dungeon_maps_amd import _native
  p = _native.Params()
  p.B, p.dc, p.vc, p.H, p.W, p.mh, p.mw = 2, 1, 0, 4, 8, 8, 8
  p.cx, p.cy, p.fx, p.fy, p.res = 3.5, 1.5, 4., 4., 0.5
  for k, v in over.items():
    setattr(p, k, v)
  return p


def _labels_call(p, dtype=3, classes=5, ws=1, ws_bytes=1 << 30):
  from dungeon_maps_amd import _native
  # (the pointers are never dereferenced: every call here is refused up front)
  return _native.lib().dm_orth_project_labels(ctypes.byref(p), 1, 1, 1, dtype, classes, None, 1, 1, None,
                                              ws, ws_bytes, None, None)


def test_c_entry_point_validates_before_any_hip_call():
  from dungeon_maps_amd import _native
  lib = _native.lib()
  err = lambda: lib.dm_last_error().decode()
  assert lib.dm_version() == _native.ABI_VERSION      # (the label entry points are additions: the number stays)
  assert _labels_call(_params(), classes=0) == -1 and "num_classes" in err()
  assert _labels_call(_params(), classes=-3) == -1 and "num_classes" in err()
  assert _labels_call(_params(dc=2)) == -1 and "one-channel" in err()
  assert _labels_call(_params(vc=5)) == -1 and "vc=5" in err()
  assert _labels_call(_params(), dtype=4) == -1 and "dtype" in err()
  assert _labels_call(_params(), dtype=-1) == -1 and "dtype" in err()
  assert _labels_call(_params(reduction=9)) == -1 and "reduction" in err()
  need = lib.dm_orth_project_labels_workspace_bytes(ctypes.byref(_params()), 3, 5)
  assert need >= 2 * 8 * 8 * 8
  assert _labels_call(_params(), ws=256, ws_bytes=need - 1) == -3 and "workspace" in err()
  assert _labels_call(_params(), ws=None, ws_bytes=need) == -3
  assert _labels_call(_params(), ws=264, ws_bytes=need) == -1 and "aligned" in err()
  assert _labels_call(_params(valid_c=1)) == -1 and "valid" in err()
  assert _labels_call(_params(B=0)) == 0                      # an empty batch is no work
  # the workspace of a refused call is 0; the compatibility route's holds the one-hot tensor
  assert lib.dm_orth_project_labels_workspace_bytes(ctypes.byref(_params()), 9, 5) == 0
  assert lib.dm_orth_project_labels_workspace_bytes(ctypes.byref(_params(dc=2)), 3, 5) == 0
  p_sum = _params(reduction=_native.REDUCE_SUM)
  assert lib.dm_orth_project_labels_workspace_bytes(ctypes.byref(p_sum), 3, 5) >= 2 * 5 * 4 * 8 * 4
  over = _native.LABEL_NATIVE_MAX_CLASSES + 1
  assert lib.dm_orth_project_labels_workspace_bytes(ctypes.byref(_params()), 3, over) >= 2 * over * 4 * 8 * 4
  assert lib.dm_labels_one_hot_f32(1, 7, 3, 1, 32, 1, None) == -1 and "dtype" in err()
  assert lib.dm_labels_one_hot_f32(1, 0, 0, 1, 32, 1, None) == -1
  assert lib.dm_labels_one_hot_f32(None, 0, 3, 1, 32, 1, None) == -1
  assert lib.dm_debug_last_label_route() == 0                 # nothing ran


def test_object_api_exposes_the_label_arguments():
  import dungeon_maps_amd as dmap
  for fn in (dmap.orth_project, dmap.MapProjector.orth_project):
    params = list(inspect.signature(fn).parameters.values())
    assert [p.name for p in params[-2:]] == ["label_map", "num_classes"]
    assert all(p.default is None for p in params[-2:])
  for meth in ("step", "plot", "reset"):
    fn = getattr(dmap.MapBuilder, meth)
    # the reference's signatures end in **kwargs: the two arguments travel in it
    assert list(inspect.signature(fn).parameters.values())[-1].kind is inspect.Parameter.VAR_KEYWORD
    inspect.signature(fn).bind(None, DEPTH, label_map=LABELS, num_classes=3)
  assert "label_map" in dmap.MapBuilder.plot.__doc__


def test_builder_forwards_labels_and_keeps_them_out_of_the_projector(monkeypatch):
  import dungeon_maps_amd as dmap
  seen = {}

  def fake(self, **kw):
    seen.update(kw)
    z = torch.zeros((1, 3, 8, 8))
    return z, z.bool(), z

  monkeypatch.setattr(dmap.MapProjector, "orth_project", fake)
  proj = dmap.MapProjector(width=8, height=4, hfov=1.2, cam_pitch=0., cam_height=1., width_offset=4.,
                           height_offset=4., map_res=0.5, map_width=8, map_height=8)
  build = dmap.MapBuilder(map_projector=proj)
  for call in (build.plot, lambda **kw: build.step(merge=False, **kw), build.reset):
    seen.clear()
    local = call(depth_map=DEPTH, label_map=LABELS, num_classes=3, map_res=0.25)
    assert seen["label_map"] is LABELS and seen["num_classes"] == 3 and seen["value_map"] is None
    assert local.proj.map_res == 0.25 and not hasattr(local.proj, "label_map")
    assert not local.is_height_map
