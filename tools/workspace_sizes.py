"""The sizes the library asks callers to allocate, over a fixed seeded sweep, as JSON (no GPU needed).

Sizes are an observable of the C ABI: callers allocate by them.  A change of the host code that is meant
to leave them alone is checked by running this against both builds and comparing the output as text:

  DUNGEON_MAPS_AMD_LIB=<the other build's libdungeon_maps_amd.so> python tools/workspace_sizes.py > a.json
  python tools/workspace_sizes.py > b.json && cmp a.json b.json

One row per line: the parameters, then dm_orth_project_workspace_bytes ("project"),
dm_frames_prepared_bytes ("prepared") and dm_orth_project_labels_workspace_bytes for each class count
("labels"; 0 for rows with a value map); at the end the rows of dm_scatter_workspace_bytes.
The sweep reaches every branch of the sizing: vc of 0, 1, 2 and >= 3 with dc == 1 (pixel list) and dc == vc,
map widths that are not a multiple of four (padded route), shapes the window path refuses (generic only),
all five reductions (mean adds counts), B of 0, 1, 64 and above the 64 frames of one launch, labels with
fewer and more than 63 classes and with sum.
"""
import itertools, json, os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dungeon_maps_amd import _native

INTS = ("B", "dc", "vc", "H", "W", "mh", "mw", "clip_border", "flip_h", "to_global", "reduction", "has_dmin",
        "has_dmax", "has_hmax", "valid_c")
LABEL_CLASSES = (1, 5, 63, 64, 200)


def params(B, dc, vc, H, W, mh, mw, reduction, fill=0.0, bounds=True, clip=0, valid_c=0, hmax=False, res=0.03):
  return dict(B=B, dc=dc, vc=vc, H=H, W=W, mh=mh, mw=mw, clip_border=clip, flip_h=1, to_global=1,
              reduction=reduction, has_dmin=int(bounds), has_dmax=int(bounds), has_hmax=int(hmax), valid_c=valid_c,
              cx=(W - 1) / 2.0, cy=(H - 1) / 2.0, fx=W / 1.4, fy=W / 1.4, res=res, fill=fill, dmin=0.15,
              dmax=5.05, hmax=1.5)


def sweep():
  rows = []
  channels = [(1, 0), (3, 0), (1, 1), (1, 2), (2, 2), (1, 3), (3, 3), (1, 40), (40, 40)]      # (dc, vc)
  shapes = [(480, 640, 512, 512), (120, 160, 241, 241), (70, 50, 96, 130), (64, 64, 1024, 1020)]
  for (dc, vc), (H, W, mh, mw), B, red in itertools.product(channels, shapes, (0, 1, 64, 65, 200), range(5)):
    rows.append(params(B, dc, vc, H, W, mh, mw, red, fill=float("-inf") if red == 0 else 0.0))
  # shapes the window path refuses (generic only): a NaN fill, a map wider than a 16-bit window, 2^28 cells;
  # no depth bounds (no strip plan); an odd width whose padded map the window path refuses too (prod)
  for B, (dc, vc), red in itertools.product((1, 64, 65), ((1, 0), (1, 3), (2, 2)), (0, 1, 3)):
    rows.append(params(B, dc, vc, 120, 160, 256, 256, red, fill=float("nan")))
    rows.append(params(B, dc, vc, 120, 160, 8, 32772, red))
    rows.append(params(B, dc, vc, 120, 160, 16384, 16384, red))
    rows.append(params(B, dc, vc, 120, 160, 256, 256, red, bounds=False))
    rows.append(params(B, dc, vc, 120, 160, 241, 241, 4))
    rows.append(params(B, dc, vc, 480, 640, 512, 512, red, clip=8, valid_c=1, hmax=True))
    rows.append(params(B, dc, vc, 480, 642, 512, 512, red))                 # (an image width the strips refuse)
    rows.append(params(B, dc, vc, 480, 640, 2048, 2048, red, res=0.005))    # (windows beyond LDS)
    rows.append(params(B, dc, vc, 240, 320, 512, 512, red, fill=-0.0))      # (labels: the compat route)
  rng = random.Random(20240611)
  for _ in range(400):
    dc, vc = rng.choice(channels)
    rows.append(params(rng.choice((0, 1, 2, 7, 64, 65, 130)), dc, vc, rng.randrange(1, 500), rng.randrange(1, 700),
                       rng.randrange(1, 700), rng.randrange(1, 700), rng.randrange(5),
                       fill=rng.choice((0.0, -1.0, float("-inf"))), bounds=rng.random() < 0.8,
                       clip=rng.choice((0, 0, 3)), valid_c=rng.choice((0, 0, 1)), hmax=rng.random() < 0.3,
                       res=rng.choice((0.03, 0.05, 0.01))))
  return rows


def main():
  lib = _native.lib()
  lines = []
  for row in sweep():
    p = _native.Params(**row)
    sizes = dict(project=lib.dm_orth_project_workspace_bytes(p), prepared=lib.dm_frames_prepared_bytes(p))
    if row["vc"] == 0 and row["dc"] == 1:
      sizes["labels"] = [lib.dm_orth_project_labels_workspace_bytes(p, _native.LABEL_DTYPE_CODE["int32"], c)
                         for c in LABEL_CLASSES]
    shown = {k: (row[k] if k in INTS else repr(row[k])) for k in row}
    lines.append(json.dumps(dict(shown, **sizes)))
  for R, C, M, has_fill, red in itertools.product((0, 1, 64, 3000), (1, 3), (1, 1000, 1 << 20), (0, 1), range(5)):
    lines.append(json.dumps(dict(R=R, C=C, M=M, has_fill=has_fill, reduction=red,
                                 scatter=lib.dm_scatter_workspace_bytes(R, C, M, has_fill, red))))
  print("[\n" + ",\n".join(lines) + "\n]")
  print(f"{len(lines)} rows", file=sys.stderr)


if __name__ == "__main__":
  main()
