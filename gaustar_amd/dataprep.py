"""A sequence's inputs before frame 0 on the GPU (data_process/ahq2gaustar.py): the rectified images and the coloured base
mesh, and the COLMAP files written from it.

Everything downstream assumes images whose principal point sits at the image centre (gsr_rig.h's rig_project projects with
W / 2, H / 2; mesh_depth renders with the centre principal point), and a first mesh that carries vertex colours
(SurfaceGaussians.from_mesh raises without them, as the reference's constructor asserts, sugar_model.py:242).  The reference
makes both with cv2 and trimesh, which are not dependencies of this project.  Here (include/gsr.h, gsr_prep.hip):

    img = rectify_image(image, intr, dist=None, border=0)             # ahq2gaustar.py:50-81, cmr_convert.py:71-109, :214-223
    sums = view_color_sums(verts, rig, images, depths=None, faces=None)   # [V,4] int32 (r, g, b, n), this rank's shard (:140-151)
    cols = finish_colors(sums, faces, fill_sweeps=8)                  # MeshColors: means, bytes, filled unseen vertices (:157-158)
    cols = color_mesh_from_views(verts, faces, rig, images)           # both; the sums all-reduced when world > 1
    save_init_mesh(path, verts, faces, cols.rgb)                      # init_mesh_{res}.obj: `v x y z r g b` with u8 / 255 (:159-160)
    write_colmap(dir, rig, verts, rgb)                                # cameras.txt, images.txt, points3D.ply (:163-244)
    prepare_first_frame(source_dir, mesh_dir, gstar_dir, frame_0, frame_end)   # the file driver, :247-287's order

The rules are stated once in gsr_prep.hip's header and restated in numpy in tests/prep_ref.py; the kernels are f64 in a fixed
order and accumulate in integers, so every result is bitwise reproducible and the colour sums do not depend on the order of
the cameras, on views_in_flight or on the sharding over ranks.

Stated departures from the reference:
  * rectify_image undistorts and centres the principal point in ONE bilinear resampling in f64; cv2 interpolates with 5-bit
    fixed-point weights and the reference resamples twice (cv2.undistort, then cv2.warpAffine).  cv2 is not available, so
    parity with its images is not pinned.
  * The reference leaves NaN colours on vertices no camera saw and lets trimesh cast them.  finish_colors fills them from their
    coloured neighbours, sweep by sweep (MeshColors.filled_at says when), and gives the rest default_color;
    fill_sweeps=0 keeps the reference's seen set (MeshColors.mean is the reference's quotient, NaN included).
  * A colour byte is the mean rounded half up in integers, (2 sum + n) / (2 n).
  * The rectified images are written as PNG (formats.save_png_rgb8), not JPEG: JPEG encoding is out of scope.  Source images
    are read with PIL where it imports, otherwise only PNG sources can be read.
Out of scope: `add_color_to_pc` (colours from a textured mesh's UV atlas), `pcl_to_depth_map.py`, cmr_convert's calibration-CSV
reader (it needs the ActorsHQ package) and JPEG encoding.
"""
from __future__ import annotations

import ctypes
import os
import struct
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Union

import numpy as np
import torch

from . import _host, _lib, _meshargs as _ma, _rig, formats, mesh_depth, sweep
from ._lib import ptr as _p

THRESHOLD = 0.005                  # ahq2gaustar.py:149
MAX_CAMERAS = 8_000_000            # 255 C < 2^31: a channel's sum over the cameras fits an int32
MAX_FILL_SWEEPS = 254              # filled_at is a byte and 255 means "never filled"
DEFAULT_COLOR = (128, 128, 128)


@dataclass
class MeshColors:
    """rgb [V,3] uint8: the vertex colours; mean [V,3] f64: sum / n as the reference forms it, NaN where no camera saw the
    vertex; count [V] int32: the cameras that saw it; filled_at [V] uint8: 0 = seen, s = filled in sweep s, 255 = default_color;
    n_unseen: vertices no camera saw; n_unfilled: vertices that got default_color."""
    rgb: torch.Tensor
    mean: torch.Tensor
    count: torch.Tensor
    filled_at: torch.Tensor
    n_unseen: int
    n_unfilled: int


# ---------------------------------------------------------------------------------------------- images
@torch.no_grad()
def rectify_image(image, intr, dist=None, border=0, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """image [H,W] or [H,W,C] uint8 (numpy or torch, C in {1, 3, 4}) resampled so that its principal point sits at
    (W / 2, H / 2): -> uint8 tensor of the same shape on the device.  intr [3,3]: fx, fy and the principal point intr[:2, 2] are
    read.  dist: None or (k1, k2, p1, p2, k3), OpenCV's order; all zero is the plain translation of img_translate.  border: a
    scalar or C values, what pixels outside the source show (cv2's BORDER_CONSTANT).  out: a contiguous uint8 tensor of the
    image's shape on the device, written in place (any alignment; it must not be `image` itself).  Runs on the current stream
    without a host read."""
    img = _ma.tensor_of(image)
    if img.dtype != torch.uint8 or img.dim() not in (2, 3):
        raise ValueError(f"image must be [H,W] or [H,W,C] uint8, got {img.dtype} {tuple(img.shape)}")
    H, W = int(img.shape[0]), int(img.shape[1])
    C = int(img.shape[2]) if img.dim() == 3 else 1
    if C not in (1, 3, 4):
        raise ValueError(f"image must have 1, 3 or 4 channels, got {C}")
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise ValueError(f"image size {(H, W)} must be positive with H W < 2^31")
    K = np.asarray(intr, np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"intr must be [3,3], got {K.shape}")
    cam4 = (ctypes.c_double * 4)(K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    dist5 = None
    if dist is not None:
        d = np.asarray(dist, np.float64).reshape(-1)
        if d.shape != (5,):
            raise ValueError(f"dist must hold k1, k2, p1, p2, k3, got {d.size} values")
        dist5 = (ctypes.c_double * 5)(*d)
    b = np.asarray(border).reshape(-1)
    if b.size not in (1, C) or (b < 0).any() or (b > 255).any() or (b != np.floor(b)).any():
        raise ValueError(f"border must be one byte value or {C} of them")
    bytes_c = (ctypes.c_ubyte * C)(*[int(x) for x in np.broadcast_to(b, (C,))])
    if device is None and out is not None and not img.is_cuda:
        device = out.device
    dev = _host.resolve_device(device, img, what="rectify_image")
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != tuple(img.shape) or out.device != dev or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {tuple(img.shape)} on {dev}")
    with _host.on_device(dev):
        src = img.to(dev).contiguous()
        if out is None:
            out = torch.empty_like(src)
        if out.data_ptr() == src.data_ptr():
            raise ValueError("out must not be the image itself")
        _lib.check(_lib.load().gsr_image_rectify(H, W, C, _p(src), _p(out), cam4, dist5, bytes_c, _host.stream_of(out)), "gsr_image_rectify")
    return out


# ---------------------------------------------------------------------------------------------- colours
_RIG_CHECKS = dict(min_side=1, max_cameras=MAX_CAMERAS)      # what _rig.Rig.of checks beyond the layout
_IMAGE = ((3,), (torch.uint8,))          # (tail, dtypes) of _rig.check_images / fetch_image
_DEPTH = ((), (torch.float32,))


@torch.no_grad()
def view_color_sums(verts, rig: dict, images, depths=None, faces=None, threshold: float = THRESHOLD, views_in_flight: int = 2,
                    rank: Optional[int] = None, world: Optional[int] = None, device=None) -> torch.Tensor:
    """sums [V,4] int32 on the device: per vertex the sum of the pixels (r, g, b) it projects to and the number of cameras, over
    the cameras of this rank's shard (sweep.camera_shard) that see it (ahq2gaustar.py:140-151): valid lookup and
    |lz - depth| < threshold.  rig: the `cmr` dict (_rig.py); the images are rectified ones, the principal point is not read.
    images: [C,H,W,3] uint8 RGB (numpy or torch) or a callable i -> [H,W,3]; depths: [C,H,W] f32 or a callable i -> [H,W];
    None renders them from (verts, faces) with mesh_depth at the centre principal point, which is what the reference's pipeline
    does in two steps through files.  Integer sums: the same bits for every views_in_flight, and all ranks' shards add up."""
    lib = _lib.load()
    rig = _rig.Rig.of(rig, **_RIG_CHECKS)
    _rig.check_images(images, rig, *_IMAGE, "image", stack_only=True)
    if depths is not None:
        _rig.check_images(depths, rig, *_DEPTH, "depth", stack_only=True)
    elif faces is None:
        raise ValueError("without depths the mesh's faces are needed to render them")
    dev = _host.resolve_device(device, verts, what="mesh_depth")
    v, f = _ma.mesh_on(verts, faces, dev) if depths is None else (_ma.verts_on(verts, dev), None)
    V = int(v.shape[0])
    mine = sweep.camera_shard(rig.C, rank, world)
    with _host.on_device(dev):
        sums = torch.zeros(V, 4, dtype=torch.int32, device=dev)

    def per_camera(_j, i):
        H, W = rig.hw(i)
        img = _rig.fetch_image(images, i, (H, W), *_IMAGE, dev, "image")
        if depths is None:
            depth = mesh_depth._view(lib, v, f, rig.cam16(i), H, W, mesh_depth.ZNEAR, mesh_depth.BACKGROUND, False, 0, None).depth
        else:
            depth = _rig.fetch_image(depths, i, (H, W), *_DEPTH, dev, "depth")
        _lib.check(lib.gsr_mesh_color_view(H, W, V, _p(v), _p(img), _p(depth), rig.cam14(i), float(threshold), _p(sums),
                                           _host.stream_of(v)), "gsr_mesh_color_view")

    sweep.run_cameras(mine, per_camera, views_in_flight, dev)
    return sums


def _device_faces(faces, dev) -> torch.Tensor:
    f = _ma.tensor_of(faces)
    if f.dtype not in (torch.int32, torch.int64):
        raise ValueError("faces must be int32 or int64")
    return _ma.faces_i32(f.to(dev))


@torch.no_grad()
def finish_colors(sums: torch.Tensor, faces=None, fill_sweeps: int = 8, default_color: Sequence[int] = DEFAULT_COLOR) -> MeshColors:
    """sums [V,4] int32 on the device (view_color_sums, all ranks' added) -> MeshColors: mean = sum / n in f64 (NaN where
    n = 0), rgb = the mean rounded half up in integers, then fill_sweeps (0..254) Jacobi sweeps over the mesh's vertex
    neighbours (meshes.MeshTopology.vertex_neighbours of faces [F,3]) in which a vertex without a colour takes the half-up
    mean of its coloured neighbours; what is left gets default_color.  faces may be None when fill_sweeps = 0.  One host read
    at the end: the two counters."""
    fill_sweeps = int(fill_sweeps)
    if not 0 <= fill_sweeps <= MAX_FILL_SWEEPS:
        raise ValueError(f"fill_sweeps must lie in 0..{MAX_FILL_SWEEPS}, got {fill_sweeps}")
    if not isinstance(sums, torch.Tensor) or sums.dim() != 2 or sums.shape[1] != 4 or sums.dtype != torch.int32 or sums.device.type != "cuda":
        raise ValueError("sums must be [V,4] int32 on a GPU")
    dc = np.asarray(default_color).reshape(-1)
    if dc.shape != (3,) or (dc < 0).any() or (dc > 255).any() or (dc != np.floor(dc)).any():
        raise ValueError("default_color must be three byte values")
    if fill_sweeps > 0 and faces is None:
        raise ValueError("filling needs the mesh's faces")
    dev, V = sums.device, int(sums.shape[0])
    lib = _lib.load()
    with _host.on_device(dev):
        sums = sums.contiguous()
        off = nbr = None
        if fill_sweeps > 0:
            from .meshes import MeshTopology
            f = _device_faces(faces, dev)
            off, nbr = MeshTopology.of(f, V).vertex_neighbours
        mean = torch.empty(V, 3, dtype=torch.float64, device=dev)
        rgb = torch.empty(V, 3, dtype=torch.uint8, device=dev)
        filled_at = torch.empty(V, dtype=torch.uint8, device=dev)
        counters = torch.zeros(2, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.gsr_mesh_color_workspace_bytes(V)) // 4, dtype=torch.int32, device=dev)
        _lib.check(lib.gsr_mesh_color_finish(V, _p(sums), _p(off), _p(nbr), fill_sweeps, (ctypes.c_ubyte * 3)(*[int(x) for x in dc]), _p(ws),
                                             _p(mean), _p(rgb), _p(filled_at), _p(counters), _host.stream_of(sums)), "gsr_mesh_color_finish")
        count = sums[:, 3].contiguous()
        n_unseen, n_unfilled = (int(x) for x in counters.cpu())
    return MeshColors(rgb, mean, count, filled_at, n_unseen, n_unfilled)


@torch.no_grad()
def color_mesh_from_views(verts, faces, rig: dict, images, depths=None, threshold: float = THRESHOLD, fill_sweeps: int = 8,
                          default_color: Sequence[int] = DEFAULT_COLOR, views_in_flight: int = 2, rank: Optional[int] = None,
                          world: Optional[int] = None, device=None) -> MeshColors:
    """compute_mesh_color (ahq2gaustar.py:124-160): view_color_sums over this rank's cameras, the sums added over the ranks
    (one all_reduce when world > 1), then finish_colors.  Every rank returns the same colours."""
    from . import dist as gdist
    fill_sweeps = int(fill_sweeps)
    if not 0 <= fill_sweeps <= MAX_FILL_SWEEPS:
        raise ValueError(f"fill_sweeps must lie in 0..{MAX_FILL_SWEEPS}, got {fill_sweeps}")
    sums = view_color_sums(verts, rig, images, depths, faces, threshold, views_in_flight, rank, world, device)
    if (gdist.world_size() if world is None else world) > 1:
        import torch.distributed as tdist
        tdist.all_reduce(sums)
    return finish_colors(sums, faces, fill_sweeps, default_color)


# ---------------------------------------------------------------------------------------------- files
def _host_array(x, dtype) -> np.ndarray:
    return np.ascontiguousarray((x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)), dtype)


def _rgb_bytes(rgb, V: int) -> np.ndarray:
    x = rgb.detach().cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    if x.dtype != np.uint8 or x.shape != (V, 3):
        raise ValueError(f"rgb must be [V,3] uint8 with V = {V}, got {x.dtype} {x.shape}")
    return x


def save_init_mesh(path, verts, faces, rgb) -> None:
    """init_mesh_{res}.obj (ahq2gaustar.py:159-160): `v x y z r g b` with the colours as u8 / 255, as
    SurfaceGaussians.save_color_mesh writes them, and `f` lines.  formats.load_obj reads the colours back exactly, and
    clip(rint(255 c)) returns the bytes."""
    v = _host_array(verts, np.float64)
    formats.save_obj(os.fspath(path), v, _host_array(faces, np.int64), _rgb_bytes(rgb, len(v)).astype(np.float64) / 255.0)


def rotmat2qvec(R) -> np.ndarray:
    """COLMAP's quaternion (qw, qx, qy, qz) of a rotation matrix, qw >= 0: the eigenvector of the largest eigenvalue of the
    symmetric 4 x 4 matrix K(R) / 3 (ahq2gaustar.py:178-189, COLMAP's read_write_model.py)."""
    R = np.asarray(R, np.float64)
    if R.shape != (3, 3):
        raise ValueError(f"R must be [3,3], got {R.shape}")
    (xx, yx, zx), (xy, yy, zy), (xz, yz, zz) = R[0], R[1], R[2]               # R[row, col] is named {col}{row}
    K = np.array([[xx - yy - zz, 0.0, 0.0, 0.0],
                  [yx + xy, yy - xx - zz, 0.0, 0.0],
                  [zx + xz, zy + yz, zz - xx - yy, 0.0],
                  [yz - zy, zx - xz, xy - yx, xx + yy + zz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    return -q if q[0] < 0 else q


def _s(x) -> str:
    return repr(float(x))           # what str() prints of a numpy float64: the shortest string that reads back


def write_colmap(folder, rig: dict, verts, rgb) -> None:
    """colmap_convert's three files (ahq2gaustar.py:163-244) in `folder` (the reference's `{frame_0:04d}/sparse/0`), created
    if missing.  cameras.txt: one PINHOLE line per camera, `i PINHOLE W H fx fy cx cy` with cx = 0.5 W, cy = 0.5 H (the images
    are rectified).  images.txt: `i qw qx qy qz tx ty tz i img_{i:04d}.jpg` and an empty line per camera (rotmat2qvec of
    extrinsics[i][:3, :3]).  points3D.ply: binary little endian, one vertex element of x y z nx ny nz (float, normals zero) and
    red green blue (uchar), written with struct / numpy as plyfile would."""
    rig = _rig.Rig.of(rig, **_RIG_CHECKS)
    intr, extr, C = rig.intr, rig.extr, rig.C
    v = _host_array(verts, np.float64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"verts must be [V,3], got {v.shape}")
    c = _rgb_bytes(rgb, len(v))
    folder = os.fspath(folder)
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "cameras.txt"), "w") as fh:
        fh.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[fx,fy,cx,cy]\n"
                 f"# Number of cameras: {C}\n")
        for i in range(C):
            H, W = rig.hw(i)
            fh.write(" ".join([str(i), "PINHOLE", str(W), str(H), _s(intr[i][0, 0]), _s(intr[i][1, 1]), _s(W * 0.5), _s(H * 0.5)]) + "\n")
    with open(os.path.join(folder, "images.txt"), "w") as fh:
        fh.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                 f"#   POINTS2D[] as (X, Y, POINT3D_ID)\n# Number of images: {C}, mean observations per image: 0\n")
        for i in range(C):
            q, t = rotmat2qvec(extr[i][:3, :3]), extr[i][:3, 3]
            fh.write(" ".join([str(i), *map(_s, q), *map(_s, t), str(i), f"img_{i:04d}.jpg"]) + "\n\n")
    rec = np.zeros(len(v), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                  ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k, name in enumerate(("x", "y", "z")):
        rec[name] = v[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rec[name] = c[:, k]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v)
    header += "".join(f"property float {n}\n" for n in ("x", "y", "z", "nx", "ny", "nz"))
    header += "".join(f"property uchar {n}\n" for n in ("red", "green", "blue")) + "end_header\n"
    assert rec.dtype.itemsize == struct.calcsize("<6f3B")
    with open(os.path.join(folder, "points3D.ply"), "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rec.tobytes())


def load_image_rgb8(path) -> np.ndarray:
    """[H,W,3] uint8 RGB of an image file: with PIL where it imports (JPEG, PNG, ...), otherwise PNG only
    (formats.load_png_rgb8)."""
    path = os.fspath(path)
    try:
        from PIL import Image
    except ImportError:
        if not path.lower().endswith(".png"):
            raise ValueError(f"{path}: without PIL only PNG images can be read") from None
        return formats.load_png_rgb8(path)
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)      # (a copy: PIL's own buffer is read-only)


def actorshq_image_path(source_dir) -> Callable[[int, int], str]:
    """(camera index, frame) -> `rgbs/Cam{c+1:03d}/Cam{c+1:03d}_rgb{f:06d}.jpg` under source_dir (ahq2gaustar.py:78-79), or the
    same name with `.png` where only that exists."""
    root = os.fspath(source_dir)

    def path(c: int, f: int) -> str:
        name = f"Cam{c + 1:03d}"
        jpg = os.path.join(root, "rgbs", name, f"{name}_rgb{f:06d}.jpg")
        png = jpg[:-4] + ".png"
        return png if os.path.exists(png) and not os.path.exists(jpg) else jpg
    return path


def prepare_first_frame(source_dir, mesh_dir, gstar_dir, frame_0: int = 0, frame_end: int = 0, interval: int = 1, res: str = "100k",
                        image_path: Union[None, Callable[[int, int], str]] = None, border=0, threshold: float = THRESHOLD,
                        fill_sweeps: int = 8, default_color: Sequence[int] = DEFAULT_COLOR, views_in_flight: int = 2) -> MeshColors:
    """ahq2gaustar.py:247-287 after cmr_convert, in its order, on files.  gstar_dir must hold `rgb_cameras.npz` (ids,
    intrinsics, extrinsics, shape, optionally dist_coeffs [C,5]; the calibration-CSV reader is out of scope).
      1. rgb_convert: for every frame f in range(frame_0, frame_end, interval) and camera c the source image image_path(c, f)
         (default: actorshq_image_path(source_dir)) is rectified -- undistorted too where dist_coeffs are not zero -- and
         written to `{f:04d}/images/img_{c:04d}.png` (PNG where the reference writes JPEG);
      2. mesh_depth.render_mesh_depth_files(wo_cxcy=True, from_humanrf=True): the depth maps and masks of
         `mesh_{f:06d}_smooth_{res}.obj` under mesh_dir;
      3. compute_mesh_color: frame_0's mesh is coloured from frame_0's rectified images and written to `init_mesh_{res}.obj`;
      4. colmap_convert: `{frame_0:04d}/sparse/0/{cameras.txt, images.txt, points3D.ply}`.
    Returns the MeshColors of step 3."""
    root = os.fspath(gstar_dir)
    cam_path = os.path.join(root, "rgb_cameras.npz")
    rig, info = _rig.Rig.load(cam_path, **_RIG_CHECKS)
    intr, C = rig.intr, rig.C
    dist = np.asarray(info["dist_coeffs"], np.float64) if "dist_coeffs" in info else None
    if dist is not None and dist.shape != (C, 5):
        raise ValueError(f"{cam_path}: dist_coeffs must be [{C},5], got {dist.shape}")
    image_path = actorshq_image_path(source_dir) if image_path is None else image_path
    frames = list(range(int(frame_0), int(frame_end), int(interval)))
    if not frames:
        raise ValueError("no frame in range(frame_0, frame_end, interval)")
    for f in frames:
        os.makedirs(os.path.join(root, f"{f:04d}/images"), exist_ok=True)
        for c in range(C):
            src = load_image_rgb8(image_path(c, f))
            if src.shape[:2] != rig.hw(c):
                raise ValueError(f"{image_path(c, f)}: {src.shape[:2]} but the camera's shape is {rig.hw(c)}")
            img = rectify_image(src, intr[c], None if dist is None else dist[c], border)
            formats.save_png_rgb8(os.path.join(root, f"{f:04d}/images/img_{c:04d}.png"), img.cpu().numpy())
    mesh_depth.render_mesh_depth_files(cam_path, mesh_dir, root, wo_cxcy=True, from_humanrf=True, mesh_res=res, frame_0=frames[0],
                                       frame_end=int(frame_end), interval=int(interval), views_in_flight=views_in_flight)
    verts, faces, _ = formats.load_obj(os.path.join(os.fspath(mesh_dir), f"mesh_{frames[0]:06d}_smooth_{res}.obj"))

    def depth_of(c: int) -> np.ndarray:
        with np.load(os.path.join(root, f"{frames[0]:04d}/depth_humanrf/img_{c:04d}_depth.npz")) as z:
            return z["depth"]

    def image_of(c: int) -> np.ndarray:      # (read back from the files, as the reference does: a rig's images need not fit)
        return formats.load_png_rgb8(os.path.join(root, f"{frames[0]:04d}/images/img_{c:04d}.png"))

    cols = color_mesh_from_views(verts, faces, rig, image_of, depth_of, threshold, fill_sweeps, default_color, views_in_flight,
                                 rank=0, world=1)
    save_init_mesh(os.path.join(root, f"init_mesh_{res}.obj"), verts, faces, cols.rgb)
    write_colmap(os.path.join(root, f"{frames[0]:04d}/sparse/0"), rig, verts, cols.rgb)
    return cols


__all__ = ["MeshColors", "rectify_image", "view_color_sums", "finish_colors", "color_mesh_from_views", "save_init_mesh",
           "rotmat2qvec", "write_colmap", "load_image_rgb8", "actorshq_image_path", "prepare_first_frame"]
