"""numpy restatement of the data-preparation kernels (gaustar_amd/csrc/gsr_prep.hip), operation by operation, and the scenes of
their tests.  Everything is float64 in the kernels' order (numpy does not contract a * b + c into an FMA; the kernels are
compiled with contraction off), and everything that is accumulated is an integer.

rectify: for output pixel (row r, column c), everything in double:
  Plain path, taken iff dist5 is null or all five coefficients are exactly 0:
    su = c + (cx - 0.5 W), sv = r + (cy - 0.5 H).
    This is img_translate's dst(c) = src(c + dx).
  Distorted path:
    x = (c - 0.5 W) / fx, y = (r - 0.5 H) / fy, r2 = x x + y y.
    rad = 1 + r2 (k1 + r2 (k2 + r2 k3)).
    xd = x rad + (2 p1 x y + p2 (r2 + 2 x x)).
    yd = y rad + (p1 (r2 + 2 y y) + 2 p2 x y).
    su = fx xd + cx, sv = fy yd + cy.
  Bilinear sampling:
    x0 = floor(su), ax = su - x0, likewise y0, ay.
    The four taps are src where inside the image and border[ch] where outside (cv2's BORDER_CONSTANT).
    If su or sv is not finite or outside the int range, the pixel is border.
    Value = (t00 (1 - ax) + t01 ax) (1 - ay) + (t10 (1 - ax) + t11 ax) ay.
    Stored as (uint8) rint(value), half to even.
  (Products left to right; "outside the int range" is outside [-2^31, 2^31 - 1).)

view_sums: per vertex rig_project (local = R p + t, row = fy (ly / lz) + H / 2, col = fx (lx / lz) + W / 2), row and column by
  rig_query (int(pix + 0.5) truncated toward zero, valid iff clipping to the image changes nothing),
  visible = valid && |lz - (double)depth[row, col]| < threshold; a visible vertex adds (r, g, b, 1) of its pixel.

finish: mean = sum / (double)n (NaN where n = 0); rgb = (2 sum + n) / (2 n) in integers; filled_at = 0 where n > 0.  Sweep
  s = 1, 2, ...: a vertex without a colour after sweep s - 1 with k > 0 coloured neighbours takes (2 S + k) / (2 k) of their rgb
  per channel and filled_at = s; a sweep reads only the previous sweep's state.  The rest: default_color, filled_at = 255."""
import numpy as np

import meshdepth_ref

INT_MIN = -2 ** 31


# ---------------------------------------------------------------------------------------------- the restatement
def rectify(src, cam4, dist=None, border=0):
    """src [H,W] or [H,W,C] uint8; cam4 = (fx, fy, cx, cy); dist = None or (k1, k2, p1, p2, k3); border: a scalar or C values."""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    flat = src.ndim == 2
    img = src[:, :, None] if flat else src
    H, W, C = img.shape
    fx, fy, cx, cy = (float(v) for v in cam4)
    bord = np.broadcast_to(np.asarray(border, np.float64).reshape(-1), (C,))
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        if dist is None or all(float(d) == 0.0 for d in dist):
            su = c + (cx - 0.5 * W)
            sv = r + (cy - 0.5 * H)
        else:
            k1, k2, p1, p2, k3 = (float(d) for d in dist)
            x = (c - 0.5 * W) / fx
            y = (r - 0.5 * H) / fy
            r2 = x * x + y * y
            rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            xd = x * rad + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
            yd = y * rad + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
            su = fx * xd + cx
            sv = fy * yd + cy
        ok = (su >= -2147483648.0) & (su < 2147483647.0) & (sv >= -2147483648.0) & (sv < 2147483647.0)   # (NaN: False)
    su, sv = np.where(ok, su, 0.0), np.where(ok, sv, 0.0)
    fx0, fy0 = np.floor(su), np.floor(sv)
    ax, ay = su - fx0, sv - fy0
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    out = np.zeros((H, W, C), np.uint8)
    for ch in range(C):
        def tap(yy, xx):
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            return np.where(inside, img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), ch].astype(np.float64), bord[ch])
        t00, t01, t10, t11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
        value = (t00 * (1.0 - ax) + t01 * ax) * (1.0 - ay) + (t10 * (1.0 - ax) + t11 * ax) * ay
        out[:, :, ch] = np.where(ok, np.rint(value), bord[ch]).astype(np.uint8)
    return out[:, :, 0] if flat else out


def rig_query(pix, n):
    """gsr_rig.h's rig_query: -> (index in [0, n - 1], valid)."""
    y = pix + 0.5
    inside = (y > -2147483649.0) & (y < 2147483648.0)                 # (NaN: False)
    p = np.where(inside, np.trunc(np.where(inside, y, 0.0)), float(INT_MIN)).astype(np.int64)
    c = np.clip(p, 0, n - 1)
    return c, p == c


def view_sums(verts, image, depth, extr, intr, threshold=0.005):
    """One camera's contribution [V,4] int64 (r, g, b, n).  image [H,W,3] uint8, depth [H,W] f32."""
    p = np.asarray(verts, np.float64)
    H, W = depth.shape
    R, t = np.asarray(extr, np.float64)[:3, :3].reshape(-1), np.asarray(extr, np.float64)[:3, 3]
    fx, fy = float(intr[0][0]), float(intr[1][1])
    with np.errstate(all="ignore"):
        lx = R[0] * p[:, 0] + R[1] * p[:, 1] + R[2] * p[:, 2] + t[0]
        ly = R[3] * p[:, 0] + R[4] * p[:, 1] + R[5] * p[:, 2] + t[1]
        lz = R[6] * p[:, 0] + R[7] * p[:, 1] + R[8] * p[:, 2] + t[2]
        pr = fy * (ly / lz) + H * 0.5
        pc = fx * (lx / lz) + W * 0.5
        row, ok_r = rig_query(pr, H)
        col, ok_c = rig_query(pc, W)
        visible = ok_r & ok_c & (np.abs(lz - depth[row, col].astype(np.float64)) < threshold)
    out = np.zeros((len(p), 4), np.int64)
    out[visible, :3] = image[row[visible], col[visible]].astype(np.int64)
    out[visible, 3] = 1
    return out


def neighbours_of_faces(faces, V):
    """trimesh's vertex_neighbors as sorted lists."""
    sets = [set() for _ in range(V)]
    for a, b, c in np.asarray(faces, np.int64).tolist():
        sets[a].update((b, c))
        sets[b].update((a, c))
        sets[c].update((a, b))
    return [sorted(s - {v}) for v, s in enumerate(sets)]


def finish(sums, neighbours, fill_sweeps=8, default_color=(128, 128, 128)):
    """sums [V,4] integers; neighbours: a list of V index lists -> dict(mean, rgb, count, filled_at, n_unseen, n_unfilled,
    reached): reached[s] = coloured vertices after sweep s (reached[0] = seen)."""
    sums = np.asarray(sums).astype(np.int64)
    S, n = sums[:, :3], sums[:, 3]
    with np.errstate(all="ignore"):
        mean = S.astype(np.float64) / n.astype(np.float64)[:, None]
    seen = n > 0
    rgb = np.zeros((len(n), 3), np.int64)
    rgb[seen] = (2 * S[seen] + n[seen, None]) // (2 * n[seen, None])
    filled_at = np.where(seen, 0, 255).astype(np.int64)
    reached = [int(seen.sum())]
    for s in range(1, fill_sweeps + 1):
        prev_rgb, prev_at = rgb.copy(), filled_at.copy()
        for v in np.nonzero(prev_at == 255)[0]:
            js = [j for j in neighbours[v] if prev_at[j] != 255]
            k = len(js)
            if k:
                rgb[v] = (2 * prev_rgb[js].sum(0) + k) // (2 * k)
                filled_at[v] = s
        reached.append(int((filled_at != 255).sum()))
    left = filled_at == 255
    rgb[left] = np.asarray(default_color, np.int64)
    return dict(mean=mean, rgb=rgb.astype(np.uint8), count=n.astype(np.int32), filled_at=filled_at.astype(np.uint8),
                n_unseen=int((~seen).sum()), n_unfilled=int(left.sum()), reached=reached)


# ---------------------------------------------------------------------------------------------- the scenes of the tests
H, W = 96, 128


def hash_image(cam, h, w, channels=3):
    """[h,w,channels] uint8: a fixed hash of (camera, row, column, channel)."""
    r, c, ch = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(channels, dtype=np.uint64), indexing="ij")
    m = np.uint64(0xFFFFFFFF)
    x = (np.uint64(cam + 1) * np.uint64(0x9E3779B1) + r * np.uint64(0x85EBCA77) + c * np.uint64(0xC2B2AE3D) + ch * np.uint64(0x27D4EB2F)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & m
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & m
    x ^= x >> np.uint64(15)
    return (x & np.uint64(255)).astype(np.uint8)


def sphere():
    from gaustar_amd import scene
    v, f = scene.icosphere(3, 0.12)
    return np.asarray(v, np.float64), np.asarray(f, np.int64)


def rig_of(angles_deg):
    """The cmr dict of cameras at eye_k = (3 cos a_k, 0.9 (-1)^k, 3 sin a_k) looking at the origin, 128 x 96, focal 1000."""
    from gaustar_amd import scene
    extr, intr = [], []
    for k, a in enumerate(angles_deg):
        a = np.deg2rad(float(a))
        eye = (3.0 * np.cos(a), 0.9 * (-1.0) ** k, 3.0 * np.sin(a))
        e, i = meshdepth_ref.camera_of(scene.look_at_camera(eye, (0.0, 0.0, 0.0), W, H, focal_px=1000.0))
        extr.append(e)
        intr.append(i)
    n = len(extr)
    return {"extrinsics": np.stack(extr), "intrinsics": np.stack(intr), "shape": np.array([[H, W]] * n, np.int32)}


FULL_RIG_ANGLES = (0, 60, 120, 180, 240, 300)
HALF_RIG_ANGLES = (-40, 0, 40)


def rig_case(angles_deg):
    """-> dict(verts, faces, rig, images [C,H,W,3], depths [C,H,W] (meshdepth_ref.render at the centre principal point),
    per_view [C,V,4], sums [V,4] int32, neighbours)."""
    verts, faces = sphere()
    rig = rig_of(angles_deg)
    C = len(angles_deg)
    images = np.stack([hash_image(i, H, W) for i in range(C)])
    depths = np.stack([meshdepth_ref.render(verts, faces, meshdepth_ref.cam16(rig["extrinsics"][i], rig["intrinsics"][i], W / 2, H / 2),
                                            H, W)[0] for i in range(C)])
    per_view = np.stack([view_sums(verts, images[i], depths[i], rig["extrinsics"][i], rig["intrinsics"][i]) for i in range(C)])
    return dict(verts=verts, faces=faces, rig=rig, images=images, depths=depths, per_view=per_view,
                sums=per_view.sum(0).astype(np.int32), neighbours=neighbours_of_faces(faces, len(verts)))
