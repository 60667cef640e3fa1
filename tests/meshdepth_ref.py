"""numpy restatement of the mesh depth rasterizer (gaustar_amd/csrc/gsr_meshdepth.hip): one mesh, one pinhole camera.

The rules, in the kernel file's order; everything is float64, and every expression below is written with the operations and the
order of the kernel (numpy does not contract a * b + c into an FMA; the kernels are compiled with contraction off):
  camera    cam16 = R (9, row-major), t (3), fx, fy, cx, cy.  local = R p + t, x = fx * (lx / lz) + cx, y = fy * (ly / lz) + cy.
  pixels    the centre of pixel (row r, column c) is at (x, y) = (c, r).
  skipped   a face with an index outside [0, V); with any vertex at lz <= znear (counted in n_clipped); with
            area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) equal to 0 or not finite.
  coverage  E_i(c, r) = (x_k - x_j) * (r - y_j) - (y_k - y_j) * (c - x_j), (j, k) = (i + 1, i + 2) mod 3; covered iff all three
            have the sign of area or are zero.  Range per axis ceil(min) .. floor(max), clamped to the image in double; an empty
            range skips the face.
  depth     iz = (E_0 / area) / z_0 + (E_1 / area) / z_1 + (E_2 / area) / z_2, left to right; z = float32(1.0 / iz), kept iff
            finite and > 0.
  winner    the smallest key (bits(z) << 32) | face per pixel.
  outputs   depth [H,W] f32 (z or background), mask [H,W] u8 (255 / 0), face [H,W] i32 (face or -1), n_clipped.
It loops over the faces and vectorises over each face's pixel range."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def cam16(extr, intr, cx, cy):
    extr, intr = np.asarray(extr, np.float64), np.asarray(intr, np.float64)
    return np.array(list(extr[:3, :3].reshape(-1)) + list(extr[:3, 3]) + [intr[0, 0], intr[1, 1], cx, cy], np.float64)


def project(cam, p):
    """p [...,3] f64 -> (x, y, lz) by the kernel's operation order."""
    p = np.asarray(p, np.float64)
    R, t = cam[:9], cam[9:12]
    fx, fy, cx, cy = cam[12:16]
    with np.errstate(all="ignore"):
        lx = R[0] * p[..., 0] + R[1] * p[..., 1] + R[2] * p[..., 2] + t[0]
        ly = R[3] * p[..., 0] + R[4] * p[..., 1] + R[5] * p[..., 2] + t[1]
        lz = R[6] * p[..., 0] + R[7] * p[..., 1] + R[8] * p[..., 2] + t[2]
        return fx * (lx / lz) + cx, fy * (ly / lz) + cy, lz


def render(verts, faces, cam, H, W, znear=0.01, background=100.0):
    """-> depth [H,W] f32, mask [H,W] u8, face [H,W] i32, n_clipped."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(verts)
    keys = np.full((H, W), EMPTY, np.uint64)
    n_clipped = 0
    X, Y, Z = project(cam, verts) if V else (np.zeros(0),) * 3
    for f, tri in enumerate(faces):
        if tri.min() < 0 or tri.max() >= V:
            continue
        x, y, z = X[tri], Y[tri], Z[tri]
        if (z <= znear).any():
            n_clipped += 1
            continue
        with np.errstate(all="ignore"):
            area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if area == 0.0 or not np.isfinite(area):
            continue
        c_lo, c_hi = max(np.ceil(x.min()), 0.0), min(np.floor(x.max()), float(W - 1))
        r_lo, r_hi = max(np.ceil(y.min()), 0.0), min(np.floor(y.max()), float(H - 1))
        if not (c_lo <= c_hi) or not (r_lo <= r_hi):
            continue
        c_lo, c_hi, r_lo, r_hi = int(c_lo), int(c_hi), int(r_lo), int(r_hi)
        pc = np.arange(c_lo, c_hi + 1, dtype=np.float64)[None, :]
        pr = np.arange(r_lo, r_hi + 1, dtype=np.float64)[:, None]
        e0 = (x[2] - x[1]) * (pr - y[1]) - (y[2] - y[1]) * (pc - x[1])
        e1 = (x[0] - x[2]) * (pr - y[2]) - (y[0] - y[2]) * (pc - x[2])
        e2 = (x[1] - x[0]) * (pr - y[0]) - (y[1] - y[0]) * (pc - x[0])
        inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) if area > 0 else ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        with np.errstate(all="ignore"):
            iz = (e0 / area) / z[0] + (e1 / area) / z[1] + (e2 / area) / z[2]
            zf = (1.0 / iz).astype(np.float32)
        keep = inside & np.isfinite(zf) & (zf > 0)
        key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        win = keys[r_lo:r_hi + 1, c_lo:c_hi + 1]
        np.minimum(win, np.where(keep, key, EMPTY), out=win)
    hit = keys != EMPTY
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(background)).astype(np.float32)
    mask = np.where(hit, 255, 0).astype(np.uint8)
    face = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return depth, mask, face, n_clipped


# ---------------------------------------------------------------------------------------------- the scenes of the tests
def camera_of(cam):
    """(extr [4,4] COLMAP world-to-camera, intr [3,3]) in f64 of a scene.Camera."""
    extr = np.asarray(cam.viewmatrix, np.float64).T.copy()
    intr = np.array([[cam.W / (2.0 * cam.tanfovx), 0.0, cam.W / 2], [0.0, cam.H / (2.0 * cam.tanfovy), cam.H / 2], [0.0, 0.0, 1.0]])
    return extr, intr


# The hand-built cases, for the camera at the origin that looks down +z with fx = fy = 1024 on a 128 x 96 image
# (IDENTITY_CAM16): at z = 2 a pixel is 1 / 512 of a unit, so the vertices below sit at exactly representable pixels.
IDENTITY_CAM16 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1024, 1024, 64, 48], np.float64)
HAND_H, HAND_W = 96, 128


def _at(px, py, z):
    return [(px - 64.0) / 1024.0 * z, (py - 48.0) / 1024.0 * z, z]


def hand_built():
    """-> (verts [V,3] f64, faces [F,3] int64, names): face k is the case names[k].
    coincident_a / coincident_b: the same triangle twice, pixels (10,10) (20,10) (10,20) at z = 2: the lower index wins.
    zero_area: two corners on one vertex.  behind: one vertex behind the camera: counted in n_clipped and absent.
    at_centre: its corner (40, 30) is a pixel centre and every other pixel centre of that row and column lies outside it.
    off_screen: wholly left of the image.  wedge: corners 1e10 units off to the left, the tip at pixel (5.5, 48): its
    pixel range must be clamped in double (the left end is past -2^31 pixels)."""
    v, f, names = [], [], []

    def face(name, *corners):
        f.append([len(v) + k for k in range(3)])
        v.extend(corners)
        names.append(name)

    tri = (_at(10, 10, 2.0), _at(20, 10, 2.0), _at(10, 20, 2.0))
    face("coincident_a", *tri)
    face("coincident_b", *tri)
    face("zero_area", _at(60, 20, 2.0), _at(60, 20, 2.0), _at(70, 25, 2.0))
    face("behind", _at(90, 10, 2.0), _at(100, 10, 2.0), [0.0, 0.0, -1.0])
    face("at_centre", _at(40, 30, 2.0), _at(43.5, 30.25, 2.0), _at(40.25, 33.5, 2.0))
    face("off_screen", _at(-50, 10, 2.0), _at(-30, 10, 2.0), _at(-40, 30, 2.0))
    face("wedge", [-1e10, -1e10, 3.5], [-1e10, 1e10, 3.5], _at(5.5, 48, 3.5))
    return np.array(v, np.float64), np.array(f, np.int64), names


def combined_mesh():
    """The mesh of the GPU comparison: a level-3 icosphere of radius 0.12 at (0, 0, 3), one triangle behind it (z = 4) whose
    projection covers the whole image and reaches ~2 000 pixels outside it, and the hand-built faces."""
    from gaustar_amd import scene
    sv, sf = scene.icosphere(3, 0.12, (0.0, 0.0, 3.0))
    hv, hf, _ = hand_built()
    bv = np.array([[-8.0, -8.0, 4.0], [8.0, -8.0, 4.0], [0.0, 16.0, 4.0]])
    verts = np.concatenate([np.asarray(sv, np.float64), bv, hv])
    faces = np.concatenate([sf, np.array([[0, 1, 2]]) + len(sv), hf + len(sv) + 3])
    return verts, faces


def combined_cameras():
    """[(cam16, H, W)]: the identity camera of hand_built() at 128 x 96, and two look-at cameras at 67 x 45 (no multiple of a
    wave, of four pixels or of 64 rows), the second with a principal point off the centre."""
    from gaustar_amd import scene
    out = [(IDENTITY_CAM16.copy(), HAND_H, HAND_W)]
    for eye, focal, pp in (((0.4, -0.3, 0.0), 500.0, (33.5, 22.5)), ((-0.5, 0.2, 0.3), 420.0, (30.25, 25.0))):
        extr, intr = camera_of(scene.look_at_camera(eye, (0.0, 0.0, 3.0), 67, 45, focal_px=focal))
        out.append((cam16(extr, intr, *pp), 45, 67))
    return out


def sphere_case(level, H=96, W=128, shift=0.0):
    """CPU test 2 / GPU test 4: icosphere(level) of radius 0.12 at the origin seen by look_at_camera((0.4, -0.3, 3), origin,
    128, 96, focal 1000) -> (verts, faces, extr, intr, (cx, cy))."""
    from gaustar_amd import scene
    v, f = scene.icosphere(level, 0.12)
    extr, intr = camera_of(scene.look_at_camera((0.4, -0.3, 3.0), (0.0, 0.0, 0.0), W, H, focal_px=1000.0))
    return np.asarray(v, np.float64), f, extr, intr, (W / 2 + shift, H / 2 + shift)


def consumer_errors(verts, extr, intr, pp, depth, mask):
    """For every vertex of the origin-centred sphere whose camera-space normal has z < -0.5: the pixel it queries by
    int(pix + 0.5) (rig_query) -> (all of them masked, max |lz - depth[pixel]|): warp_mesh.py:294-295's visibility test."""
    cam = cam16(extr, intr, *pp)
    x, y, lz = project(cam, verts)
    n = verts / np.linalg.norm(verts, axis=1, keepdims=True)
    nz = n @ np.asarray(extr, np.float64)[2, :3]
    sel = nz < -0.5
    r, c = (y[sel] + 0.5).astype(np.int32), (x[sel] + 0.5).astype(np.int32)
    assert sel.sum() > 10 and (r >= 0).all() and (r < depth.shape[0]).all() and (c >= 0).all() and (c < depth.shape[1]).all()
    return bool((mask[r, c] == 255).all()), float(np.abs(lz[sel] - depth[r, c].astype(np.float64)).max())
