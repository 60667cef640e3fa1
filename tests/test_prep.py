"""The data-preparation rules (gsr_prep.hip) checked on their numpy restatement tests/prep_ref.py, the COLMAP writer, the RGB
PNG pair and the C ABI's argument checks -- all without a GPU.  tests/test_gpu_prep.py compares the kernels with the same
restatement bit for bit."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import prep_ref as ref
from conftest import ROOT
from gaustar_amd import dataprep, formats


def _image(h, w, c, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


@pytest.mark.parametrize("dx,dy", [(3, -2), (-5, 4), (0, 0)])
def test_integer_shift_is_a_padded_copy(dx, dy):
    """img_translate's dst(r, c) = src(r + dy, c + dx), the border where that is outside."""
    h, w = 9, 13
    src = _image(h, w, 3)
    border = (7, 200, 33)
    got = ref.rectify(src, (50.0, 50.0, w / 2 + dx, h / 2 + dy), None, border)
    want = np.empty_like(src)
    want[:] = np.asarray(border, np.uint8)
    for r in range(h):
        for c in range(w):
            if 0 <= r + dy < h and 0 <= c + dx < w:
                want[r, c] = src[r + dy, c + dx]
    assert np.array_equal(got, want)
    assert np.array_equal(ref.rectify(src, (50.0, 50.0, w / 2 + dx, h / 2 + dy), (0.0,) * 5, border), want)      # all zero: the plain path
    assert np.array_equal(ref.rectify(src[:, :, 0], (50.0, 50.0, w / 2 + dx, h / 2 + dy), None, 7), want[:, :, 0])


def test_a_shift_larger_than_the_image_is_all_border():
    h, w = 9, 13
    src = _image(h, w, 4, seed=1)
    border = (1, 2, 3, 250)
    for cx, cy in ((w / 2 + w + 0.5, h / 2), (w / 2, h / 2 - h - 3.25), (1e300, 0.0), (float("nan"), 0.0), (float("inf"), 0.0)):
        got = ref.rectify(src, (50.0, 50.0, cx, cy), None, border)
        assert (got == np.asarray(border, np.uint8)).all(), (cx, cy)


def test_half_pixel_shift_rounds_half_to_even():
    src = np.array([[0, 1, 4, 7]], np.uint8)                 # means 0.5, 2.5, 5.5 -> 0, 2, 6; the last blends with the border 9: 8
    got = ref.rectify(src, (1.0, 1.0, 2.0 + 0.5, 0.5), None, 9)
    assert got.tolist() == [[0, 2, 6, 8]]


PATH_NEIGHBOURS = [[1], [0, 2], [1, 3], [2, 4], [3]]        # seen, unseen, unseen, unseen, seen


def test_finish_on_a_path_graph():
    # vertex 0: sums over 2 cameras, the red mean 101 / 2 = 50.5 rounds half up to 51; vertex 4: one camera
    sums = np.array([[101, 20, 7, 2], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [200, 41, 9, 1]])
    one = ref.finish(sums, PATH_NEIGHBOURS, 1, (1, 2, 3))
    assert one["filled_at"].tolist() == [0, 1, 255, 1, 0]
    assert one["rgb"].tolist() == [[51, 10, 4], [51, 10, 4], [1, 2, 3], [200, 41, 9], [200, 41, 9]]
    assert (one["n_unseen"], one["n_unfilled"]) == (3, 1) and one["reached"] == [2, 4]
    two = ref.finish(sums, PATH_NEIGHBOURS, 2, (1, 2, 3))
    assert two["filled_at"].tolist() == [0, 1, 2, 1, 0]
    # vertex 2 takes the half-up mean of vertices 1 and 3: (51 + 200) / 2 = 125.5 -> 126, (10 + 41) / 2 = 25.5 -> 26, 13 / 2 -> 7
    assert two["rgb"].tolist() == [[51, 10, 4], [51, 10, 4], [126, 26, 7], [200, 41, 9], [200, 41, 9]]
    assert (two["n_unseen"], two["n_unfilled"]) == (3, 0)
    zero = ref.finish(sums, PATH_NEIGHBOURS, 0, (1, 2, 3))
    assert zero["filled_at"].tolist() == [0, 255, 255, 255, 0] and zero["n_unfilled"] == 3
    assert zero["mean"][0].tolist() == [50.5, 10.0, 3.5] and np.isnan(zero["mean"][1:4]).all() and zero["count"].tolist() == [2, 0, 0, 0, 1]


def test_rotmat2qvec_of_known_rotations():
    s = np.sqrt(0.5)
    rz90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert np.allclose(dataprep.rotmat2qvec(rz90), [s, 0.0, 0.0, s], atol=1e-15)
    assert np.allclose(dataprep.rotmat2qvec(np.eye(3)), [1.0, 0.0, 0.0, 0.0], atol=1e-15)
    # 240 degrees about (1, 1, 1) / sqrt(3): the half angle's cosine is negative, so the quaternion is flipped to qw >= 0
    r240 = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    q = dataprep.rotmat2qvec(r240)
    assert q[0] >= 0 and np.allclose(q, [0.5, -0.5, -0.5, -0.5], atol=1e-15)


def test_write_colmap_files(tmp_path):
    s = float(np.sqrt(0.5))
    extr = np.stack([np.eye(4), np.eye(4)])
    extr[0, :3, 3] = [0.25, -1.5, 3.0]
    extr[1, :3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    extr[1, :3, 3] = [1.0, 2.0, 0.125]
    intr = np.array([[[1000.5, 0, 70.25], [0, 990.0, 40.0], [0, 0, 1]], [[800.0, 0, 1.0], [0, 801.25, 2.0], [0, 0, 1]]])
    rig = {"extrinsics": extr, "intrinsics": intr, "shape": np.array([[96, 128], [45, 67]], np.int32)}
    verts = np.array([[0.1, 0.2, 0.3], [-1.0, 2.5, 1e-3]])
    rgb = np.array([[1, 2, 3], [255, 0, 128]], np.uint8)
    folder = tmp_path / "0004" / "sparse" / "0"
    dataprep.write_colmap(folder, rig, verts, rgb)
    assert sorted(os.listdir(folder)) == ["cameras.txt", "images.txt", "points3D.ply"]
    assert (folder / "cameras.txt").read_text() == (
        "# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[fx,fy,cx,cy]\n# Number of cameras: 2\n"
        "0 PINHOLE 128 96 1000.5 990.0 64.0 48.0\n1 PINHOLE 67 45 800.0 801.25 33.5 22.5\n")
    q1 = dataprep.rotmat2qvec(extr[1, :3, :3])
    assert q1[0] >= 0 and np.allclose(q1, [s, 0, 0, s], atol=1e-15)
    assert (folder / "images.txt").read_text() == (
        "# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
        "#   POINTS2D[] as (X, Y, POINT3D_ID)\n# Number of images: 2, mean observations per image: 0\n"
        "0 1.0 0.0 0.0 0.0 0.25 -1.5 3.0 0 img_0000.jpg\n\n"
        "1 " + " ".join(repr(float(x)) for x in q1) + " 1.0 2.0 0.125 1 img_0001.jpg\n\n")
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
              "end_header\n").encode("ascii")
    body = b"".join(struct.pack("<6f3B", *[float(x) for x in v], 0.0, 0.0, 0.0, *[int(x) for x in c]) for v, c in zip(verts, rgb))
    assert (folder / "points3D.ply").read_bytes() == header + body
    with pytest.raises(ValueError):
        dataprep.write_colmap(folder, rig, verts, rgb.astype(np.float32))


def test_png_rgb8_round_trip(tmp_path):
    a = _image(5, 7, 3, seed=3)
    path = str(tmp_path / "a.png")
    formats.save_png_rgb8(path, a)
    b = formats.load_png_rgb8(path)
    assert b.dtype == np.uint8 and b.shape == (5, 7, 3) and np.array_equal(a, b)
    assert open(path, "rb").read()[25] == 2                   # IHDR's colour type
    with pytest.raises(ValueError):
        formats.save_png_rgb8(path, a[:, :, 0])
    with pytest.raises(ValueError):
        formats.load_png_gray8(path)
    formats.save_png_gray8(path, a[:, :, 0].copy())
    with pytest.raises(ValueError):
        formats.load_png_rgb8(path)
    assert np.array_equal(dataprep.load_image_rgb8(path)[:, :, 0], a[:, :, 0]) if _has_pil() else True


def _has_pil():
    try:
        import PIL.Image  # noqa: F401
        return True
    except ImportError:
        return False


def test_save_init_mesh_round_trip(tmp_path):
    verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.1, 0.2, 0.3]])
    faces = np.array([[0, 1, 2], [1, 3, 2]])
    rgb = np.array([[0, 1, 2], [127, 128, 129], [253, 254, 255], [51, 26, 7]], np.uint8)
    path = tmp_path / "init_mesh_100k.obj"
    dataprep.save_init_mesh(path, verts, faces, rgb)
    v, f, c = formats.load_obj(str(path))
    assert np.array_equal(v, verts) and np.array_equal(f, faces) and np.array_equal(c, rgb.astype(np.float64) / 255.0)
    assert np.array_equal(np.clip(np.rint(255.0 * c.astype(np.float32)), 0, 255).astype(np.uint8), rgb)


def test_python_checks_come_before_any_launch():
    """Wrong shapes raise ValueError without a device (no tensor has been uploaded, nothing launched)."""
    rig = ref.rig_of((0, 60))
    verts = np.zeros((4, 3))
    faces = np.array([[0, 1, 2]])
    good = np.zeros((2, ref.H, ref.W, 3), np.uint8)
    with pytest.raises(ValueError):
        dataprep.view_color_sums(verts, rig, good[:, :, :-1], faces=faces)                 # H W disagrees with rig["shape"]
    with pytest.raises(ValueError):
        dataprep.view_color_sums(verts, rig, good[:1], faces=faces)                        # one image short
    with pytest.raises(ValueError):
        dataprep.view_color_sums(verts, rig, good, depths=np.zeros((2, ref.H, ref.W), np.float64))
    with pytest.raises(ValueError):
        dataprep.view_color_sums(verts, rig, good)                                         # neither depths nor faces
    with pytest.raises(ValueError):
        dataprep.rectify_image(np.zeros((4, 4, 2), np.uint8), np.eye(3))                   # C = 2
    with pytest.raises(ValueError):
        dataprep.rectify_image(np.zeros((4, 4, 3), np.float32), np.eye(3))
    with pytest.raises(ValueError):
        dataprep.rectify_image(np.zeros((4, 4, 3), np.uint8), np.eye(3), dist=(0.1, 0.2))
    with pytest.raises(ValueError):
        dataprep.rectify_image(np.zeros((4, 4, 3), np.uint8), np.eye(3), border=(1, 2))
    with pytest.raises(ValueError):
        dataprep.color_mesh_from_views(verts, faces, rig, good, fill_sweeps=255)
    with pytest.raises(ValueError):
        dataprep.finish_colors(np.zeros((4, 4), np.int32), faces, fill_sweeps=255)


def test_abi_declares_and_validates_without_gpu(hip_lib):
    from gaustar_amd import _lib
    text = open(os.path.join(ROOT, "include", "gsr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("gsr_image_rectify", "gsr_mesh_color_view", "gsr_mesh_color_workspace_bytes", "gsr_mesh_color_finish"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SIGNATURES and hasattr(hip_lib, name)
    for cite in ("ahq2gaustar.py:50-81", "cmr_convert.py:71-109", "ahq2gaustar.py:124-160"):
        assert cite in text
    assert hip_lib.gsr_abi_version() == 16 and _lib.ABI_VERSION == 16
    assert hip_lib.gsr_mesh_color_workspace_bytes(1000) == 12000 and hip_lib.gsr_mesh_color_workspace_bytes(0) == 0
    buf = (ctypes.c_double * 64)()                           # host memory: every check below fails before any device work
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 256)
    cam4 = (ctypes.c_double * 4)(50.0, 50.0, 2.0, 2.0)
    dist = (ctypes.c_double * 5)()
    border = (ctypes.c_ubyte * 4)()
    order = ("H", "W", "C", "src", "dst", "cam", "dist", "border", "stream")
    rect = lambda **kw: hip_lib.gsr_image_rectify(*[{**dict(H=4, W=4, C=3, src=p, dst=q, cam=cam4, dist=dist, border=border, stream=None),
                                                     **kw}[k] for k in order])
    for missing in ("src", "dst", "cam", "border"):
        assert rect(**{missing: None}) != 0 and b"null" in hip_lib.gsr_last_error(), missing
    assert rect(C=2) != 0 and b"C must be 1, 3 or 4" in hip_lib.gsr_last_error()
    assert rect(dst=p) != 0 and b"dst must not be src" in hip_lib.gsr_last_error()
    assert rect(H=0) != 0 and b"positive" in hip_lib.gsr_last_error()
    assert rect(H=1 << 16, W=1 << 15) != 0 and b"too large" in hip_lib.gsr_last_error()
    cam14 = (ctypes.c_double * 14)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 50, 50)
    order = ("H", "W", "V", "verts", "image", "depth", "cam", "thr", "sums", "stream")
    view = lambda **kw: hip_lib.gsr_mesh_color_view(*[{**dict(H=4, W=4, V=3, verts=p, image=p, depth=p, cam=cam14, thr=0.005, sums=p,
                                                              stream=None), **kw}[k] for k in order])
    for missing in ("verts", "image", "depth", "cam", "sums"):
        assert view(**{missing: None}) != 0 and b"null" in hip_lib.gsr_last_error(), missing
    assert view(H=0) != 0 and b"positive" in hip_lib.gsr_last_error()
    assert view(V=0, verts=None, sums=None) == 0
    dc = (ctypes.c_ubyte * 3)(128, 128, 128)
    order = ("V", "sums", "off", "nbr", "sweeps", "dc", "ws", "mean", "rgb", "at", "cnt", "stream")
    fin = lambda **kw: hip_lib.gsr_mesh_color_finish(*[{**dict(V=3, sums=p, off=p, nbr=p, sweeps=2, dc=dc, ws=p, mean=p, rgb=p, at=p, cnt=p,
                                                               stream=None), **kw}[k] for k in order])
    for missing in ("sums", "off", "nbr", "dc", "ws", "mean", "rgb", "at", "cnt"):
        assert fin(**{missing: None}) != 0 and b"null" in hip_lib.gsr_last_error(), missing
    assert fin(sweeps=255) != 0 and b"fill_sweeps" in hip_lib.gsr_last_error()
    assert fin(sweeps=-1) != 0 and b"fill_sweeps" in hip_lib.gsr_last_error()
    assert fin(V=-1) != 0 and b"negative" in hip_lib.gsr_last_error()
    assert fin(V=0, sums=None, ws=None, mean=None, rgb=None, at=None, cnt=None) == 0
