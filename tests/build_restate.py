"""The index build of a cloud (rescan_amd/csrc/rs_cloud_api.hip: cloud_create_impl, rs_build.hip, rs_buildplan.h) restated in numpy: float32
where the code uses float, float64 where it uses double, one step per function in the build's own order.  plan() returns what
capi.Cloud.layout() returns, to be compared for equality of integers and bits.

clamped=False restates the trial grids as they stood before rs_buildplan.h (±Inf wins the bounds and resets its axis to [0, 0]; a
point's trial cell is clamped from below only).  It is a witness for tests/test_hard_build_cpu.py, nothing else uses it.
"""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
TRIAL_CELLS_MAX = 1073741824.0
TABLE_CELLS_MAX = 48.0e6
TABLE_DIM_MAX = 16777216.0
TRIAL_ATTEMPTS = 8
OUT_OF_RANGE = 1 << 64            # what stands for the undefined conversion of +Inf or of a float beyond 2^64


def switches():
    """(RS_HIP_AUTO_CELL_SCALE, RS_HIP_TILE_EXTENT_MAX) as the library would use them now, as floats"""
    from rescan_amd import capi
    return F(capi.switch_get("RS_HIP_AUTO_CELL_SCALE")), F(capi.switch_get("RS_HIP_TILE_EXTENT_MAX"))


def _err():
    return np.errstate(all="ignore")


def bounds(pos, finite_only=True):
    """(mn, mx) float32: over the finite coordinates of each axis; an axis without one gets [0, 0]"""
    mn, mx = np.zeros(3, F), np.zeros(3, F)
    for a in range(3):
        v = pos[:, a]
        v = v[np.isfinite(v)] if finite_only else v[~np.isnan(v)]
        if len(v) and np.isfinite(v.min()) and np.isfinite(v.max()):
            mn[a], mx[a] = v.min(), v.max()
    return mn, mx


def trial_first_cell(mn, mx):
    with _err():
        ext = max(mx - mn)
        q = F(ext / F(64.0))
    lo = q if q > F(1e-4) else F(1e-4)
    return lo if lo < F(0.1) else F(0.1)


def trial_grid(mn, mx, c0):
    """dict(inv, cells, countable, td, top, words) of the trial grid with cell c0"""
    with _err():
        inv = F(1.0) / F(c0)
        f = np.floor((mx - mn) * inv)
    f = np.where(f >= 0, f, F(0.0)).astype(F)
    d = f.astype(np.float64) + 2.0
    with _err():
        cells = 1.0 * d[0] * d[1] * d[2]
    g = dict(inv=inv, cells=cells, countable=bool(cells <= TRIAL_CELLS_MAX), td=None, top=None, words=0)
    if g["countable"]:
        g["td"] = [int(x) for x in d]
        top = np.array([F(t - 1) for t in g["td"]], F)
        for a in range(3):
            if np.float64(top[a]) > d[a] - 1.0:
                top[a] = np.nextafter(top[a], F(0.0))
        g["top"] = top
        g["words"] = int(cells / 32.0) + 2
    return g


def trial_ids(pos, mn, g, clamped=True):
    """every point's cell id in a countable trial grid, as Python integers (OUT_OF_RANGE: no defined value)"""
    with _err():
        c = np.floor((pos - mn[None, :]) * g["inv"]).astype(F)
    if clamped:
        c = np.where(c >= 0, c, F(0.0)).astype(F)
        c = np.where(c > g["top"][None, :], g["top"][None, :], c).astype(F)
        c = c.astype(np.uint64)
        return [(int(a) * g["td"][1] + int(b)) * g["td"][2] + int(z) for a, b, z in c]
    c = np.where(c > 0, c, F(0.0)).astype(np.float64)              # fmaxf(0, c): NaN and everything negative give 0
    out = []
    for row in c:
        if (row >= 2.0 ** 64).any():
            out.append(OUT_OF_RANGE)
        else:
            a, b, z = (int(x) for x in row)
            out.append(((a * g["td"][1] + b) * g["td"][2] + z) % (1 << 64))
    return out


def per_cell(n, occ):
    return F(n) / F(max(1, occ))


def auto_cell_of(pc, c0):
    return F(F(2.0) * F(c0)) / np.sqrt(pc if pc > F(1.0) else F(1.0), dtype=F)


def auto_cell(pos, mn, mx, scale, clamped=True, trace=None):
    """the density-derived cell of n > 0 points; trace (a list) receives (attempt, c0, grid, ids) of every counted trial grid"""
    n = len(pos)
    c0 = trial_first_cell(mn, mx)
    cell = F(0.1)
    for attempt in range(TRIAL_ATTEMPTS):
        g = trial_grid(mn, mx, c0)
        if not g["countable"] and attempt < TRIAL_ATTEMPTS - 1:
            c0 = F(c0 * F(2.0))
            continue
        pc = F(4.0)
        if g["countable"]:
            ids = trial_ids(pos, mn, g, clamped)
            if trace is not None:
                trace.append((attempt, c0, g, ids))
            pc = per_cell(n, len(set(ids)))
        if pc >= F(4.0) or attempt == TRIAL_ATTEMPTS - 1:
            cell = auto_cell_of(pc, c0)
            break
        c0 = F(c0 * F(2.0))
    s = F(cell * F(scale))
    lo = s if s > F(0.005) else F(0.005)
    return lo if lo < F(2.0) else F(2.0)


def table_dims(mn, mx, cell):
    """(cell, dims): the cell doubled until the table has at most 48e6 cells and 2^24 along every axis; an axis has the cells of its
    extent, counted in double, and never fewer than the float cell of its maximum.  None: no table (an extent that overflows a float)"""
    cell = F(cell)
    with _err():
        if not np.isfinite(mx - mn).all():
            return None
    while True:
        with _err():
            inv = F(1.0) / cell
            if not inv > 0:
                return None
            d = np.floor((mx.astype(np.float64) - mn.astype(np.float64)) / np.float64(cell)) + 1.0
            f = np.floor((mx - mn) * inv).astype(np.float64) + 1.0
            d = np.maximum(d, f)
            cells = 1.0 * d[0] * d[1] * d[2]
        if cells <= TABLE_CELLS_MAX and (d <= TABLE_DIM_MAX).all():
            return cell, d.astype(np.int32)
        with _err():
            cell = F(cell * F(2.0))


def cell_coords(pos, mn, inv_cell, dims):
    """(n, 3) int64: cell_of_dev of every coordinate"""
    with _err():
        c = np.floor((pos - mn[None, :]) * F(inv_cell)).astype(F)
    c = np.where(c >= 0, c, F(0.0)).astype(F)
    top = (dims - 1).astype(F)
    c = np.where(c > top[None, :], top[None, :], c)
    return c.astype(np.int64)


def cell_ids(pos, mn, inv_cell, dims):
    c = cell_coords(pos, mn, inv_cell, dims)
    return (c[:, 2] * int(dims[1]) + c[:, 1]) * int(dims[0]) + c[:, 0]


def hilbert3(x, y, z, bits):
    """Skilling's transpose form, as hilbert3_dev: uint32 arrays in, the index on the curve out"""
    X = [np.array(v, np.uint32).copy() for v in (x, y, z)]
    M = np.uint32(1 << (bits - 1))
    Q = int(M)
    while Q > 1:
        P = np.uint32(Q - 1)
        for i in range(3):
            hit = (X[i] & np.uint32(Q)) != 0
            t = np.where(hit, np.uint32(0), (X[0] ^ X[i]) & P).astype(np.uint32)      # (i == 0: t is 0)
            X[0] = np.where(hit, X[0] ^ P, X[0] ^ t).astype(np.uint32)
            if i:
                X[i] = (X[i] ^ t).astype(np.uint32)
        Q >>= 1
    X[1] ^= X[0]; X[2] ^= X[1]
    t = np.zeros_like(X[0])
    Q = int(M)
    while Q > 1:
        t = np.where((X[2] & np.uint32(Q)) != 0, t ^ np.uint32(Q - 1), t).astype(np.uint32)
        Q >>= 1
    for i in range(3):
        X[i] ^= t
    h = np.zeros_like(X[0])
    for b in range(bits - 1, -1, -1):
        for i in range(3):
            h = ((h << np.uint32(1)) | ((X[i] >> np.uint32(b)) & np.uint32(1))).astype(np.uint32)
    return h


def hilbert_scale(mn, mx):
    ext = F(0.0)
    with _err():
        e = mx - mn
    for a in range(3):
        if np.isfinite(e[a]) and e[a] > ext:
            ext = e[a]
    with _err():
        return F(1024.0) / ext if ext > 0 else F(0.0)


def hilbert_cells(pos, mn, scale):
    with _err():
        f = ((pos - mn[None, :]) * F(scale)).astype(F)
    f = np.where(f >= 0, f, F(0.0)).astype(F)
    f = np.where(f > F(1023.0), F(1023.0), f)
    return f.astype(np.uint32)


def hilbert_keys(pos, mn, scale):
    c = hilbert_cells(pos, mn, scale)
    return hilbert3(c[:, 0], c[:, 1], c[:, 2], 10)


def brute_occupied(n, mn, mx):
    vol = 1.0
    for a in range(3):
        vol *= np.floor((np.float64(mx[a]) - np.float64(mn[a])) / 0.1) + 1.0
    return int(max(1.0, min(float(n), float(np.power(vol, 2.0 / 3.0)))))


def extent_limit(n, occupied, cell, extent_max):
    if n <= 0 or occupied == 0 or not cell > 0:
        return FLT_MAX
    pc = F(n) / F(occupied)
    spacing = F(cell) / np.sqrt(pc if pc > F(1.0) else F(1.0), dtype=F)
    want = F(F(12.0) * spacing)
    lo = want if want > F(0.25) else F(0.25)
    return F(extent_max) if F(extent_max) < lo else lo


def _fmin(a, b):
    return b if a != a else (a if (b != b or a <= b) else b)       # fminf: a NaN loses


def _fmax(a, b):
    return b if a != a else (a if (b != b or a >= b) else b)


def greedy_tiles(q, limit):
    """Sequentially, as the comment above k_build_tile_next states it: a tile ends after 64 points or when adding the next point
    would stretch its bounding box beyond `limit` on any axis.  q: (n, 3) float32 in Hilbert order.  Returns the tile starts + [n].
    (Minima and maxima of float32 values as Python floats, which is exact; the box's extent by a float32 subtraction.)"""
    n, limit = len(q), F(limit)
    pts = q.astype(np.float64).tolist()
    starts = []
    s = 0
    with _err():
        while s < n:
            starts.append(s)
            lo, hi = list(pts[s]), list(pts[s])
            e = s + 1
            while e < n and e - s < 64:
                p = pts[e]
                nlo = [_fmin(lo[a], p[a]) for a in range(3)]
                nhi = [_fmax(hi[a], p[a]) for a in range(3)]
                if F(nhi[0]) - F(nlo[0]) > limit or F(nhi[1]) - F(nlo[1]) > limit or F(nhi[2]) - F(nlo[2]) > limit:
                    break
                lo, hi = nlo, nhi
                e += 1
            s = e
    return np.array(starts + [n], np.uint32)


def records(a, order):
    """the 16-byte records of `a` (n, 3) float32 in the given order: its bits, and the original index in the fourth word"""
    r = np.zeros((len(order), 4), np.uint32)
    if len(order):
        r[:, :3] = a[order].view(np.uint32)
        r[:, 3] = order
    return r


def plan(pos, cell_size=-1.0, nor=None, scale=None, extent_max=None, limit=None, clamped=True):
    """What capi.Cloud(pos, nor, cell_size).layout() returns.  limit: tile against this limit, not the restated one (the brute
    layout's goes through pow)."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    n = len(pos)
    if scale is None or extent_max is None:
        scale, extent_max = switches()
    cell_size = F(cell_size)
    mn, mx = bounds(pos, finite_only=clamped) if n else (np.zeros(3, F), np.zeros(3, F))
    trials = []
    if cell_size < 0:
        cell_size = auto_cell(pos, mn, mx, scale, clamped, trials) if n else F(0.1)
    chosen = cell_size                                   # (given or derived, before the table is sized)
    dims, inv_cell, cell = np.ones(3, np.int32), F(0.0), cell_size
    if cell_size > 0 and n > 0:
        t = table_dims(mn, mx, cell_size)
        if t is None:
            cell_size = cell = F(0.0)
        else:
            cell, dims = t
            inv_cell = F(1.0) / cell
    n_cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    ids = cell_ids(pos, mn, inv_cell, dims) if n else np.zeros(0, np.int64)
    assert not n or (0 <= ids.min() and ids.max() < n_cells)
    order = np.argsort(ids, kind="stable").astype(np.int32)
    cell_start = np.zeros(n_cells + 1, np.uint32)
    if n:
        np.cumsum(np.bincount(ids, minlength=n_cells), out=cell_start[1:], dtype=np.uint32)
    occupied = len(np.unique(ids))
    lim_cell = cell if cell_size > 0 else F(0.1)
    if not cell_size > 0:
        occupied = brute_occupied(n, mn, mx)
    want_limit = extent_limit(n, occupied, lim_cell, extent_max)
    if limit is None:
        limit = want_limit
    scale_h = hilbert_scale(mn, mx)
    keys = hilbert_keys(pos, mn, scale_h) if n else np.zeros(0, np.uint32)
    assert not n or keys.max() < (1 << 30)
    qorder = np.argsort(keys, kind="stable").astype(np.int32)
    by_orig = np.zeros(n, np.int32); by_orig[qorder] = np.arange(n, dtype=np.int32)
    tiles = greedy_tiles(pos[qorder], limit) if n else np.zeros(1, np.uint32)
    out = dict(min=mn, cell=F(cell if inv_cell > 0 else 0.0), inv_cell=inv_cell, dims=dims, n=n, n_cells=n_cells, occupied=int(occupied),
               extent_limit=F(limit), restated_limit=F(want_limit), n_tiles=len(tiles) - 1, cell_start=cell_start, order=order, qorder=qorder,
               tiles=tiles, by_orig=by_orig, pos=records(pos, order), qpos=records(pos, qorder), keys=keys, cell_ids=ids, max=mx,
               trials=trials, cell_size=chosen, hilbert_scale=scale_h)
    if nor is not None:
        nor = np.ascontiguousarray(nor, F).reshape(-1, 3)
        out["nor"] = records(nor, order); out["nor"][:, 3] = 0
        out["qnor"] = records(nor, qorder); out["qnor"][:, 3] = 0
    return out


SCALARS = ("cell", "inv_cell", "n", "n_cells", "occupied", "extent_limit", "n_tiles")
ARRAYS = ("dims", "cell_start", "order", "qorder", "tiles", "by_orig", "pos", "qpos")


def assert_layout(got, want, what="", skip=()):
    """every scalar and every array of a layout equals the restatement's: integers and bits.  (min by value: the sign of a zero
    minimum is whichever of -0.0 and +0.0 the bounds' atomics met last, and no index depends on it.)"""
    assert (np.asarray(got["min"], F) == np.asarray(want["min"], F)).all(), (what, "min", got["min"], want["min"])
    for k in SCALARS:
        if k in skip:
            continue
        a, b = got[k], want[k]
        if isinstance(b, np.floating):
            a, b = F(a).view(np.uint32), F(b).view(np.uint32)
        assert a == b, (what, k, got[k], want[k])
    names = ARRAYS + (("nor", "qnor") if "nor" in want else ())
    for k in names:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0] if a.size else []
        assert not len(bad), (what, k, f"{len(bad)} rows differ, first {bad[0]}", a[bad[0]], b[bad[0]])


def layout_bytes(L):
    """one bytes object of everything in a layout() (for layouts that must be equal to the byte)"""
    keys = sorted(k for k in L if k != "min")
    return b"".join(np.asarray(L[k]).tobytes() for k in keys) + (np.asarray(L["min"], F) + F(0.0)).tobytes()
