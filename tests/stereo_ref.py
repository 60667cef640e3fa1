"""numpy restatement of plane-sweep stereo behind a prior (gaustar_amd/csrc/gsr_stereo.hip behind gaustar_amd.stereo) for
tests/test_stereo.py and tests/test_gpu_stereo.py: luma, the relative pose, the sweep, the consistency pass and the merge, and
the scene the tests share -- a textured sphere with a dent that no silhouette sees.

The rules are those include/gsr.h states; every float expression below has the kernel's operations in the kernel's order, in
explicit adds (no np.sum, no BLAS; numpy does not contract a * b + c, the kernels are compiled with contraction off).  sweep()
works a plane at a time over the whole image; sweep_brute() states rules 4 to 8 pixel by pixel in Python floats from the
rules' text alone, and consistency_brute() rule 9, for tiny images."""
import functools
import math

import numpy as np

import hull_ref as hr
import meshdepth_ref as mr

ZNEAR = 0.01
f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ luma, cameras, poses
def luma(rgb):
    """[H,W,3] uint8 -> [H,W] uint8: (77 R + 150 G + 29 B + 128) >> 8."""
    c = np.asarray(rgb).astype(np.int64)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def relative_pose(extr_r, extr_s):
    """(R_sr [3,3], t_sr [3]): R_sr = R_s R_r^T, t_sr = t_s - R_sr t_r, each element three products added as (a + b) + c."""
    Er, Es = np.asarray(extr_r, f64), np.asarray(extr_s, f64)
    R, t = np.zeros((3, 3)), np.zeros(3)
    for i in range(3):
        for j in range(3):
            R[i, j] = (Es[i, 0] * Er[j, 0] + Es[i, 1] * Er[j, 1]) + Es[i, 2] * Er[j, 2]
    for i in range(3):
        t[i] = Es[i, 3] - ((R[i, 0] * Er[0, 3] + R[i, 1] * Er[1, 3]) + R[i, 2] * Er[2, 3])
    return R, t


def reference_camera(rig, r, use_principal_point=False):
    """(fx, fy, cx, cy) of camera r: the principal point at the image's centre unless use_principal_point."""
    H, W = (int(v) for v in rig["shape"][r])
    intr = np.asarray(rig["intrinsics"][r], f64)
    cx, cy = (intr[0, 2], intr[1, 2]) if use_principal_point else (W / 2, H / 2)
    return float(intr[0, 0]), float(intr[1, 1]), float(cx), float(cy)


def source_rows(rig, r, srcs, images, states=None, use_principal_point=False):
    """The camera table of reference camera r: per source its relative pose, its own intrinsics and its image (luma for the
    sweep; depth, with `states`, for the consistency pass)."""
    out = []
    for j, s in enumerate(srcs):
        R, t = relative_pose(rig["extrinsics"][r], rig["extrinsics"][s])
        fx, fy, cx, cy = reference_camera(rig, s, use_principal_point)
        out.append({"R": R, "t": t, "fx": fx, "fy": fy, "cx": cx, "cy": cy, "img": np.asarray(images[j]),
                    "state": None if states is None else np.asarray(states[j])})
    return out


def _local(src, Lx, Ly, Lz):
    R, t = src["R"], src["t"]
    lx = ((R[0, 0] * Lx + R[0, 1] * Ly) + R[0, 2] * Lz) + t[0]
    ly = ((R[1, 0] * Lx + R[1, 1] * Ly) + R[1, 2] * Lz) + t[1]
    lz = ((R[2, 0] * Lx + R[2, 1] * Ly) + R[2, 2] * Lz) + t[2]
    return lx, ly, lz


def warp(refc, src, rr, cc, z):
    """The reference pixels (rows rr, columns cc: integer arrays, on the image or off it) on the plane at depth z, seen by the
    source: the bilinear luma there as f64, -1 where the warp is invalid."""
    fx, fy, cx, cy = refc
    img = src["img"]
    Hs, Ws = img.shape
    with np.errstate(all="ignore"):
        Lx = ((cc.astype(f64) - cx) / fx) * z
        Ly = ((rr.astype(f64) - cy) / fy) * z
        lx, ly, lz = _local(src, Lx, Ly, np.full(Lx.shape, z))
        u = src["fx"] * (lx / lz) + src["cx"]
        v = src["fy"] * (ly / lz) + src["cy"]
        ok = (lz > ZNEAR) & (u >= 0.0) & (u < float(Ws - 1)) & (v >= 0.0) & (v < float(Hs - 1))
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    ax, ay = u - x0.astype(f64), v - y0.astype(f64)
    g = img.astype(f64)
    i00, i01, i10, i11 = g[y0, x0], g[y0, x0 + 1], g[y0 + 1, x0], g[y0 + 1, x0 + 1]
    w = (1.0 - ay) * ((1.0 - ax) * i00 + ax * i01) + ay * ((1.0 - ax) * i10 + ax * i11)
    return np.where(ok, w, -1.0)


# ------------------------------------------------------------------------------------------------ the sweep
def bands(prior, cfg):
    """(covered, k_lo, k_hi) per pixel; an uncovered pixel has the empty band 1 .. 0."""
    d = np.asarray(prior, f32).astype(f64)
    with np.errstate(all="ignore"):
        covered = (d > ZNEAR) & (d < cfg.background)
        k_min = math.floor(ZNEAR / cfg.step) + 1
        lo = np.ceil((np.where(covered, d, 1.0) - cfg.near) / cfg.step)
        hi = np.floor((np.where(covered, d, 1.0) + cfg.far) / cfg.step)
    k_lo = np.where(covered, np.maximum(lo, float(k_min)), 1.0).astype(np.int64)
    k_hi = np.where(covered, hi, 0.0).astype(np.int64)
    return covered, k_lo, k_hi


def sweep(gl, prior, refc, sources, cfg):
    """gl [H,W] uint8 the reference luma, prior [H,W] f32, refc = (fx, fy, cx, cy), sources = source_rows(...), cfg a resolved
    gaustar_amd.stereo.StereoConfig -> {depth f32, score f32, state uint8, plane int16}."""
    gl, prior = np.asarray(gl), np.asarray(prior, f32)
    H, W = gl.shape
    R = int(cfg.radius)
    K = 2 * R + 1
    N = K * K
    covered, k_lo, k_hi = bands(prior, cfg)
    banded = covered & (k_lo <= k_hi)
    gpad = np.pad(gl.astype(np.int64), R)
    A, B = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for dy in range(K):
        for dx in range(K):
            g = gpad[dy:dy + H, dx:dx + W]
            A = A + g
            B = B + g * g
    Vr = N * B - A * A
    thr = float(N * N) * float(cfg.min_var)
    inside = np.zeros((H, W), bool)
    if H > 2 * R and W > 2 * R:
        inside[R:H - R, R:W - R] = True
    active = banded & inside & ~(Vr.astype(f64) < thr)
    gpad = gpad.astype(f64)
    Af, Vrf = A.astype(f64), Vr.astype(f64)

    best, cm, cp, prev = (np.full((H, W), v) for v in (-2.0, 0.0, 0.0, 0.0))
    have, cm_ok, cp_ok, prev_ok = (np.zeros((H, W), bool) for _ in range(4))
    kb = np.full((H, W), -1, np.int64)
    rr, cc = np.mgrid[-R:H + R, -R:W + R]
    S = len(sources)
    planes = range(int(k_lo[banded].min()), int(k_hi[banded].max()) + 1) if banded.any() else ()
    for k in planes:
        in_band = active & (k >= k_lo) & (k <= k_hi)
        if not in_band.any():               # (every update below is under in_band)
            continue
        z = float(k) * cfg.step
        scores, v = [], np.zeros((H, W), np.int64)
        for src in sources:
            wpad = warp(refc, src, rr, cc, z)
            Sw, Sww, Swg = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
            bad = np.zeros((H, W), bool)
            for dy in range(K):
                for dx in range(K):
                    w, g = wpad[dy:dy + H, dx:dx + W], gpad[dy:dy + H, dx:dx + W]
                    bad = bad | (w < 0.0)
                    Sw = Sw + w
                    Sww = Sww + w * w
                    Swg = Swg + w * g
            Vs = float(N) * Sww - Sw * Sw
            ok = ~bad & (Vs >= thr)
            with np.errstate(all="ignore"):
                sc = (float(N) * Swg - Sw * Af) / np.sqrt(Vs * Vrf)
            scores.append(np.where(ok, sc, -2.0))
            v = v + ok
        srt = -np.sort(-np.stack(scores), axis=0)          # descending; the invalid ones (-2) last
        T = np.minimum(int(cfg.keep), v)
        cost = srt[0]
        with np.errstate(all="ignore"):             # (pixels outside their band may hold anything: masked below)
            for i in range(1, S):
                cost = np.where(i < T, cost + srt[i], cost)
            cost = cost / np.maximum(T, 1).astype(f64)
        usable = in_band & (v >= int(cfg.min_sources))
        cost = np.where(usable, cost, 0.0)
        new = usable & (~have | (cost > best))
        plus = usable & ~new & (k == kb + 1)
        cm, cm_ok, cp_ok = np.where(new, prev, cm), np.where(new, prev_ok, cm_ok), np.where(new, False, cp_ok)
        best, kb, have = np.where(new, cost, best), np.where(new, k, kb), have | new
        cp, cp_ok = np.where(plus, cost, cp), cp_ok | plus
        prev, prev_ok = np.where(in_band, cost, prev), np.where(in_band, usable, prev_ok)

    state = np.where(~covered, 0, np.where(~have, 1, np.where(best < cfg.min_score, 2, 3))).astype(np.uint8)
    den = (cm - 2.0 * best) + cp
    use = cm_ok & cp_ok & (den < 0.0)
    with np.errstate(all="ignore"):
        delta = np.where(use, np.clip((0.5 * (cm - cp)) / np.where(use, den, -1.0), -0.5, 0.5), 0.0)
    refined = ((kb.astype(f64) + delta) * cfg.step).astype(f32)
    depth = np.where(state == 3, refined.view(np.uint32), prior.view(np.uint32)).astype(np.uint32).view(f32)
    score = np.where(state >= 2, best.astype(f32), f32(-2.0)).astype(f32)
    plane = np.where(state >= 2, kb, -1).astype(np.int16)
    return {"depth": depth, "score": score, "state": state, "plane": plane}


def _warp_one(refc, src, r, c, z):
    """Rule 5 for one tap in Python floats: the warped luma, or None."""
    fx, fy, cx, cy = refc
    L = (((c - cx) / fx) * z, ((r - cy) / fy) * z, z)
    R, t = src["R"], src["t"]
    loc = [((float(R[i, 0]) * L[0] + float(R[i, 1]) * L[1]) + float(R[i, 2]) * L[2]) + float(t[i]) for i in range(3)]
    if not loc[2] > ZNEAR:
        return None
    px = src["fx"] * (loc[0] / loc[2]) + src["cx"]
    py = src["fy"] * (loc[1] / loc[2]) + src["cy"]
    if math.isnan(px) or math.isnan(py) or abs(px) > 1e9 or abs(py) > 1e9:
        return None
    img = src["img"]
    Hs, Ws = img.shape
    x0, y0 = math.floor(px), math.floor(py)
    if not (0 <= x0 <= Ws - 2 and 0 <= y0 <= Hs - 2):
        return None
    ax, ay = px - x0, py - y0
    I = lambda y, x: float(img[y, x])
    return (1.0 - ay) * ((1.0 - ax) * I(y0, x0) + ax * I(y0, x0 + 1)) + ay * ((1.0 - ax) * I(y0 + 1, x0) + ax * I(y0 + 1, x0 + 1))


def sweep_brute(gl, prior, refc, sources, cfg):
    """Rules 4 to 8 pixel by pixel, from their text: for tiny images."""
    gl, prior = np.asarray(gl), np.asarray(prior, f32)
    H, W = gl.shape
    R = int(cfg.radius)
    N = (2 * R + 1) ** 2
    out = {"depth": prior.copy(), "score": np.full((H, W), -2, f32), "state": np.zeros((H, W), np.uint8),
           "plane": np.full((H, W), -1, np.int16)}
    k_min = math.floor(ZNEAR / cfg.step) + 1
    for r in range(H):
        for c in range(W):
            d = float(prior[r, c])
            if not (ZNEAR < d < cfg.background):
                continue
            out["state"][r, c] = 1
            k_lo, k_hi = max(k_min, math.ceil((d - cfg.near) / cfg.step)), math.floor((d + cfg.far) / cfg.step)
            taps = [(r + dy, c + dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
            if any(not (0 <= y < H and 0 <= x < W) for y, x in taps):
                continue
            g = [int(gl[y, x]) for y, x in taps]
            A, B = sum(g), sum(v * v for v in g)           # (integers: exact in any order)
            Vr = N * B - A * A
            if float(Vr) < N * N * cfg.min_var:
                continue
            costs = {}
            for k in range(k_lo, k_hi + 1):
                z = k * cfg.step
                scores = []
                for src in sources:
                    ws = [_warp_one(refc, src, y, x, z) for y, x in taps]
                    if any(w is None for w in ws):
                        continue
                    Sw = Sww = Swg = 0.0
                    for w, gv in zip(ws, g):
                        Sw += w
                        Sww += w * w
                        Swg += w * float(gv)
                    Vs = N * Sww - Sw * Sw
                    if not Vs >= N * N * cfg.min_var:
                        continue
                    scores.append((N * Swg - Sw * A) / math.sqrt(Vs * float(Vr)))
                if len(scores) < cfg.min_sources:
                    continue
                scores.sort(reverse=True)
                T = min(int(cfg.keep), len(scores))
                total = scores[0]
                for x in scores[1:T]:
                    total += x
                costs[k] = total / T
            if not costs:
                continue
            ks = max(costs, key=lambda k: (costs[k], -k))
            out["score"][r, c], out["plane"][r, c] = f32(costs[ks]), ks
            if costs[ks] < cfg.min_score:
                out["state"][r, c] = 2
                continue
            delta = 0.0
            if ks - 1 in costs and ks + 1 in costs:
                den = (costs[ks - 1] - 2.0 * costs[ks]) + costs[ks + 1]
                if den < 0:
                    delta = min(0.5, max(-0.5, (0.5 * (costs[ks - 1] - costs[ks + 1])) / den))
            out["state"][r, c] = 3
            out["depth"][r, c] = f32((ks + delta) * cfg.step)
    return out


# ------------------------------------------------------------------------------------------------ consistency, merge
def consistency(refc, depth, state, sources, tol, min_consistent):
    """state [H,W] uint8 with 3 -> 4 where at least min_consistent of the sources (source_rows with depth images and the
    sweep's states) agree."""
    depth, state = np.asarray(depth, f32), np.asarray(state, np.uint8)
    H, W = state.shape
    fx, fy, cx, cy = refc
    rr, cc = np.mgrid[0:H, 0:W]
    z = depth.astype(f64)
    n = np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        Lx, Ly = ((cc.astype(f64) - cx) / fx) * z, ((rr.astype(f64) - cy) / fy) * z
        for src in sources:
            Hs, Ws = src["img"].shape
            lx, ly, lz = _local(src, Lx, Ly, z)
            yu = (src["fx"] * (lx / lz) + src["cx"]) + 0.5
            yv = (src["fy"] * (ly / lz) + src["cy"]) + 0.5
            ok = (lz > ZNEAR) & (yu > -1.0) & (yu < float(Ws)) & (yv > -1.0) & (yv < float(Hs))      # gsr_rig.h's rig_query
            col = np.trunc(np.where(ok, yu, 0.0)).astype(np.int64)
            row = np.trunc(np.where(ok, yv, 0.0)).astype(np.int64)
            diff = src["img"][row, col].astype(f64) - lz
            n = n + (ok & (src["state"][row, col] >= 3) & (np.abs(diff) <= tol))
    return np.where((state == 3) & (n >= int(min_consistent)), 4, state).astype(np.uint8)


def consistency_brute(refc, depth, state, sources, tol, min_consistent):
    """Rule 9 pixel by pixel."""
    out = np.array(state, np.uint8)
    fx, fy, cx, cy = refc
    H, W = out.shape
    for r in range(H):
        for c in range(W):
            if state[r, c] != 3:
                continue
            z = float(depth[r, c])
            L = (((c - cx) / fx) * z, ((r - cy) / fy) * z, z)
            n = 0
            for src in sources:
                R, t = src["R"], src["t"]
                loc = [((float(R[i, 0]) * L[0] + float(R[i, 1]) * L[1]) + float(R[i, 2]) * L[2]) + float(t[i]) for i in range(3)]
                if not loc[2] > ZNEAR:
                    continue
                px = src["fx"] * (loc[0] / loc[2]) + src["cx"]
                py = src["fy"] * (loc[1] / loc[2]) + src["cy"]
                if not (abs(px) < 1e9 and abs(py) < 1e9):
                    continue
                col, row = int(px + 0.5), int(py + 0.5)            # truncation toward zero
                Hs, Ws = src["img"].shape
                if not (px + 0.5 > -1 and 0 <= col < Ws and py + 0.5 > -1 and 0 <= row < Hs):
                    continue
                if src["state"][row, col] >= 3 and abs(float(src["img"][row, col]) - loc[2]) <= tol:
                    n += 1
            if n >= min_consistent:
                out[r, c] = 4
    return out


def merge(th, wh, ts, ws, cs, min_weight):
    """(tsdf, weight, color [3,...], touched [nuz,nuy,nux] bool) of two volumes' arrays over one grid."""
    carve = (ws.astype(f64) >= float(min_weight)) & (wh == 1) & (ts > th)
    t = np.where(carve, ts, th).astype(f32)
    color = np.where(ws > 0, cs, f32(0)).astype(f32)
    near = (wh == 1) & (np.abs(t) < 1)
    U = 16
    nz, ny, nx = (n // U for n in t.shape)
    return t, wh.astype(f32), color, near.reshape(nz, U, ny, U, nx, U).any(axis=(1, 3, 5))


# ------------------------------------------------------------------------------------------------ the scene
RADIUS = 0.1                                   # the sphere (hull_ref.sphere_mesh), in hull_ref.BOX with hull_ref.VOXEL
DENT_DEPTH = 5 * hr.VOXEL                      # the bump's depth at its centre: 5 voxels of the test volume
DENT_HALF_ANGLE = math.radians(40.0)
DIST, FOCAL = 0.75, 150.0                      # the cameras: the sphere is 40 pixels across, a voxel 1.6
N_CAMERAS, SPACING = 9, math.radians(18.0)     # an arc of 144 degrees in azimuth around the dent's axis
ELEVATIONS = (0.10, -0.08)
AXIS_AZIMUTH = math.radians(90.0)
BACKGROUND_GREY = 30


def dent_axis():
    return np.array([math.cos(AXIS_AZIMUTH), 0.0, math.sin(AXIS_AZIMUTH)])


def meshes():
    """(verts of the sphere, verts of the dented sphere, faces): vertices within DENT_HALF_ANGLE of the axis are pushed
    radially inward by DENT_DEPTH (1 - x^2)^2, x the angle over the half angle."""
    v, f = hr.sphere_mesh()
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    x = np.arccos(np.clip(n @ dent_axis(), -1.0, 1.0)) / DENT_HALF_ANGLE
    bump = np.where(x < 1.0, (1.0 - x * x) ** 2, 0.0)
    return v, v - n * (DENT_DEPTH * bump)[:, None], f


def eyes():
    out = []
    for i in range(N_CAMERAS):
        az, el = AXIS_AZIMUTH + (i - N_CAMERAS // 2) * SPACING, ELEVATIONS[i % 2]
        out.append(DIST * np.array([math.cos(el) * math.cos(az), math.sin(el), math.cos(el) * math.sin(az)]))
    return out


def texture(p):
    """A procedural grey value of a 3-D point: four sinusoids of incommensurate frequency (wavelengths of 4 to 11 pixels)."""
    k = np.array([[307.0, 41.0, 89.0], [-71.0, 233.0, 59.0], [53.0, -97.0, 173.0], [127.0, 113.0, -131.0]])
    ph = np.array([0.3, 1.7, 2.9, 4.1])
    s = np.sin(p @ k.T + ph)
    return 128.0 + 28.0 * (((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3])


def render_view(verts, faces, extr, fx, fy, cx, cy, H, W):
    """(image [H,W] uint8, depth [H,W] f32 with 100 where nothing is, mask [H,W] uint8) of the textured mesh in one camera."""
    extr = np.asarray(extr, f64)
    intr = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    depth, mask, _face, _n = mr.render(verts, faces, mr.cam16(extr, intr, cx, cy), H, W)
    rr, cc = np.mgrid[0:H, 0:W]
    z = depth.astype(f64)
    local = np.stack([(cc - cx) / fx * z, (rr - cy) / fy * z, z], -1)
    world = (local - extr[:3, 3]) @ extr[:3, :3]                         # R^T (local - t)
    grey = np.clip(np.rint(texture(world)), 0, 255).astype(np.uint8)
    return np.where(mask > 0, grey, np.uint8(BACKGROUND_GREY)).astype(np.uint8), depth, mask


class Scene:
    """rig, images [H,W] uint8 (grey, taken as luma), truth / prior depth maps f32 (the dented / the plain sphere), masks of
    the dented sphere, sources [C,S] (gaustar_amd.stereo.select_sources around the origin)."""


@functools.lru_cache(maxsize=None)
def scene(H=48, W=64):
    from gaustar_amd import stereo
    sc = Scene()
    plain, dented, faces = meshes()
    sc.plain, sc.dented, sc.faces = plain, dented, faces
    sc.rig = hr.look_at_rig(eyes(), (0.0, 0.0, 0.0), H, W, FOCAL)
    sc.images, sc.truth, sc.masks, sc.prior = [], [], [], []
    for i in range(N_CAMERAS):
        fx, fy, cx, cy = reference_camera(sc.rig, i)
        img, depth, mask = render_view(dented, faces, sc.rig["extrinsics"][i], fx, fy, cx, cy, H, W)
        sc.images.append(img), sc.truth.append(depth), sc.masks.append(mask)
        sc.prior.append(mr.render(plain, faces, mr.cam16(sc.rig["extrinsics"][i], sc.rig["intrinsics"][i], cx, cy), H, W)[0])
    sc.sources = stereo.select_sources(sc.rig, 4, focus=(0.0, 0.0, 0.0))
    return sc


def scene_config(**kw):
    """The config of the tests: the band reaches 15 planes behind the prior, the dent is 10 deep."""
    from gaustar_amd import stereo
    return stereo.StereoConfig(**{**dict(step=0.004, near=0.008, far=0.06), **kw})


def restated_view(sc, r, cfg, srcs=None):
    """sweep() of camera r of the scene against its sources."""
    srcs = [int(s) for s in (sc.sources[r] if srcs is None else srcs) if int(s) >= 0]
    rows = source_rows(sc.rig, r, srcs, [sc.images[s] for s in srcs])
    return sweep(sc.images[r], sc.prior[r], reference_camera(sc.rig, r), rows, cfg.resolved(len(srcs)))


def restated_consistency(sc, views, cfg):
    """consistency() over the scene's rig: the states after the second pass."""
    out = []
    for r in range(len(views)):
        srcs = [int(s) for s in sc.sources[r] if int(s) >= 0]
        c = cfg.resolved(len(srcs))
        rows = source_rows(sc.rig, r, srcs, [views[s]["depth"] for s in srcs], [views[s]["state"] for s in srcs])
        out.append(consistency(reference_camera(sc.rig, r), views[r]["depth"], views[r]["state"], rows, c.tol, c.min_consistent))
    return out


def sees(sc, r, s, tol=0.01):
    """[H,W] bool: the true surface point of camera r's pixel is seen by camera s (projects onto its image at its depth)."""
    H, W = sc.truth[r].shape
    rows = source_rows(sc.rig, r, [s], [sc.truth[s]])[0]
    fx, fy, cx, cy = reference_camera(sc.rig, r)
    rr, cc = np.mgrid[0:H, 0:W]
    z = sc.truth[r].astype(f64)
    lx, ly, lz = _local(rows, (cc - cx) / fx * z, (rr - cy) / fy * z, z)
    with np.errstate(all="ignore"):
        u, v = rows["fx"] * (lx / lz) + rows["cx"] + 0.5, rows["fy"] * (ly / lz) + rows["cy"] + 0.5
    Hs, Ws = sc.truth[s].shape
    ok = (lz > ZNEAR) & (u >= 0) & (u < Ws) & (v >= 0) & (v < Hs)
    col, row = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
    return ok & (np.abs(sc.truth[s][row, col].astype(f64) - lz) < tol)


# ------------------------------------------------------------------------------------------------ the whole chain on the CPU
HULL_RADIUS = 7                                # >= TRUNC * FOCAL / z + 0.5 over hull_ref.BOX's volume from DIST
MIN_VIEWS = 9                                  # every camera sees the whole volume


def dent_samples(sc, per_edge=8):
    """Points of the TRUE surface inside the dent's cap [n,3] f64: a barycentric lattice on every face of the dented mesh
    whose centroid lies within the cap."""
    tri = sc.dented[sc.faces]
    cen = tri.mean(1)
    cap = np.arccos(np.clip((cen / np.linalg.norm(cen, axis=1, keepdims=True)) @ dent_axis(), -1.0, 1.0)) < DENT_HALF_ANGLE
    tri = tri[cap]
    out = []
    for i in range(per_edge + 1):
        for j in range(per_edge + 1 - i):
            a, b = (i + 1 / 3) / (per_edge + 1), (j + 1 / 3) / (per_edge + 1)
            out.append(tri[:, 0] * (1 - a - b) + tri[:, 1] * a + tri[:, 2] * b)
    return np.concatenate(out)


def restated_chain(sc, cfg, min_weight=3.0):
    """hull_ref, this module and fusion_ref in refine_hull's order -> (hull verts, hull faces, refined verts, refined faces,
    per-camera final states)."""
    import fusion_ref as fr
    d2s = [hr.mask_distance(m, 128, HULL_RADIUS) for m in sc.masks]
    vol = hr.new_volume(hr.BOX[0], hr.BOX[1], hr.VOXEL, hr.TRUNC)
    hr.carve(vol, hr.rig_cameras(sc.rig, d2s))
    hr.finish(vol, MIN_VIEWS)
    hv, hf, _ = fr.marching_cubes(vol)
    C = len(sc.images)
    priors = []
    for i in range(C):
        fx, fy, cx, cy = reference_camera(sc.rig, i)
        H, W = sc.images[i].shape
        priors.append(mr.render(hv.astype(f64), hf, mr.cam16(sc.rig["extrinsics"][i], sc.rig["intrinsics"][i], cx, cy), H, W)[0])
    views = []
    for r in range(C):
        srcs = [int(s) for s in sc.sources[r] if int(s) >= 0]
        rows = source_rows(sc.rig, r, srcs, [sc.images[s] for s in srcs])
        views.append(sweep(sc.images[r], priors[r], reference_camera(sc.rig, r), rows, cfg.resolved(len(srcs))))
    states = restated_consistency(sc, views, cfg)
    svol = fr.new_volume(hr.BOX[0], hr.BOX[1], hr.VOXEL, hr.TRUNC)
    for i in range(C):
        depth = np.where(states[i] == 4, views[i]["depth"], f32(0)).astype(f32)
        rgb = np.repeat(sc.images[i][:, :, None], 3, axis=2)
        fr.integrate(svol, depth, rgb, reference_camera(sc.rig, i), sc.rig["extrinsics"][i])
    t, w, color, _touched = merge(vol["tsdf"], vol["weight"], svol["tsdf"], svol["weight"], svol["color"], min_weight)
    merged = dict(vol, tsdf=t, weight=w, color=color)
    rv, rf, _ = fr.marching_cubes(merged)
    return hv, hf, rv, rf, states


def agreement_gaps(refc, depth, src):
    """Per pixel of the reference and one source of a consistency table: (the nearest source pixel is on the image and the
    point lies beyond znear, |depth_s there - local.z| in f64) -- what consistency() compares with tol."""
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    fx, fy, cx, cy = refc
    rr, cc = np.mgrid[0:H, 0:W]
    z = depth.astype(f64)
    Hs, Ws = src["img"].shape
    with np.errstate(all="ignore"):
        lx, ly, lz = _local(src, ((cc.astype(f64) - cx) / fx) * z, ((rr.astype(f64) - cy) / fy) * z, z)
        yu, yv = (src["fx"] * (lx / lz) + src["cx"]) + 0.5, (src["fy"] * (ly / lz) + src["cy"]) + 0.5
        ok = (lz > ZNEAR) & (yu > -1.0) & (yu < float(Ws)) & (yv > -1.0) & (yv < float(Hs))
        col, row = np.trunc(np.where(ok, yu, 0.0)).astype(np.int64), np.trunc(np.where(ok, yv, 0.0)).astype(np.int64)
        return ok & (src["state"][row, col] >= 3), np.abs(src["img"][row, col].astype(f64) - lz)
