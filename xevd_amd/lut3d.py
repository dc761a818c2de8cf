"""Reader of .cube 3D LUT files (Adobe / IRIDAS .cube, and Resolve's form with a 1D block in front) for XgpuDecoder.lut3d_create.

Plumbing only: the file's numbers come back as float arrays and as the arguments of xgpu_lut3d_shaper; quantising them to the uint16 tables the kernel reads is
the C helpers' job (xgpu_lut3d_from_float, xgpu_lut3d_shaper)."""
import numpy as np

_KEYS3 = ("DOMAIN_MIN", "DOMAIN_MAX")
_KEYS2 = ("LUT_1D_INPUT_RANGE", "LUT_3D_INPUT_RANGE")


def load_cube(path):
    """-> dict(title, n, nodes float32 [n^3, 3] in file order (red fastest), curve float32 [n_1d, 3] or None, in_min, in_max (three floats each),
    shaper = None (identity) or dict(curve=, in_min=, in_max=) for xgpu_lut3d_shaper).
    Read: TITLE, LUT_3D_SIZE, an optional LUT_1D_SIZE block in front of the cube, DOMAIN_MIN / DOMAIN_MAX, LUT_1D_INPUT_RANGE / LUT_3D_INPUT_RANGE (the range of
    the first table of the file takes the place of the domain), comments (#) and blank lines.  The input range is where the shaper's t runs from 0 to 1; the 1D
    block, if any, is its curve.  A file whose 3D table sits behind a 1D block with a LUT_3D_INPUT_RANGE other than 0 1 is refused: the curve's output is the
    position in the cube.  Malformed files raise ValueError."""
    title, n3, n1 = "", None, None
    vals = {}
    rows = []
    with open(path, "r", encoding="utf-8", errors="replace") as fh:
        for ln, line in enumerate(fh, 1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            tok = line.split()
            key = tok[0].upper()
            try:
                if key == "TITLE":
                    title = line[5:].strip().strip('"')
                elif key == "LUT_3D_SIZE":
                    n3 = int(tok[1])
                elif key == "LUT_1D_SIZE":
                    n1 = int(tok[1])
                elif key in _KEYS3:
                    vals[key] = [float(v) for v in tok[1:4]]
                    if len(tok) != 4:
                        raise ValueError
                elif key in _KEYS2:
                    vals[key] = [float(v) for v in tok[1:3]]
                    if len(tok) != 3:
                        raise ValueError
                elif key[0].isalpha() and key not in ("NAN", "INF"):      # an unknown keyword (a row may start with nan or inf)
                    raise ValueError
                else:
                    if len(tok) != 3:
                        raise ValueError
                    rows.append([float(v) for v in tok])
            except (ValueError, IndexError):
                raise ValueError(f"{path}:{ln}: cannot read {line!r}") from None
    if n3 is None:
        raise ValueError(f"{path}: no LUT_3D_SIZE")
    if not 2 <= n3 <= 65:
        raise ValueError(f"{path}: LUT_3D_SIZE {n3}: 2 .. 65 nodes per axis are supported")
    if n1 is not None and n1 < 2:
        raise ValueError(f"{path}: LUT_1D_SIZE {n1}")
    want = (n1 or 0) + n3 ** 3
    if len(rows) != want:
        raise ValueError(f"{path}: {len(rows)} rows of three values, the sizes ask for {want}")
    data = np.asarray(rows, np.float32).reshape(-1, 3)
    curve = data[:n1].copy() if n1 else None
    nodes = data[n1 or 0:].copy()
    in_min, in_max = vals.get("DOMAIN_MIN", [0.0] * 3), vals.get("DOMAIN_MAX", [1.0] * 3)
    first = "LUT_1D_INPUT_RANGE" if n1 else "LUT_3D_INPUT_RANGE"
    if first in vals:
        in_min, in_max = [vals[first][0]] * 3, [vals[first][1]] * 3
    if n1 and vals.get("LUT_3D_INPUT_RANGE", [0.0, 1.0]) != [0.0, 1.0]:
        raise ValueError(f"{path}: a 1D block in front of a cube with LUT_3D_INPUT_RANGE other than 0 1 is not supported")
    if any(not hi > lo for lo, hi in zip(in_min, in_max)):
        raise ValueError(f"{path}: the input range {in_min} .. {in_max} is empty")
    identity = curve is None and in_min == [0.0] * 3 and in_max == [1.0] * 3
    shaper = None if identity else dict(curve=curve, in_min=in_min, in_max=in_max)
    return dict(title=title, n=n3, nodes=nodes, curve=curve, in_min=in_min, in_max=in_max, shaper=shaper)
