"""The mesh depth rasterizer's rules (gsr_meshdepth.hip), checked on their numpy restatement tests/meshdepth_ref.py, the grey
PNG writer, and the C ABI's argument checks -- all without a GPU.  tests/test_gpu_meshdepth.py compares the kernels with the
same restatement bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

import meshdepth_ref as ref
from conftest import ROOT
from gaustar_amd import formats, scene


def test_tilted_quad_is_the_ray_plane_intersection():
    """Two triangles of one plane, tilted in depth, cover the 128 x 96 image: every pixel is masked and the depth is the f64
    ray / plane intersection at the pixel centre rounded to f32 (relative 2^-24, plus 1e-12 for the f64 arithmetic)."""
    H, W = 96, 128
    extr, intr = ref.camera_of(scene.look_at_camera((0.4, -0.3, 3.0), (0.0, 0.0, 0.0), W, H, focal_px=1000.0))
    quad = np.array([[x, y, 0.3 * x + 0.2 * y] for x, y in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5))])
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    cam = ref.cam16(extr, intr, W / 2, H / 2)
    depth, mask, face, n_clipped = ref.render(quad, faces, cam, H, W)
    assert (mask == 255).all() and n_clipped == 0 and set(np.unique(face)) == {0, 1}
    p = quad @ extr[:3, :3].T + extr[:3, 3]                    # the plane n . p = d in camera space
    n = np.cross(p[1] - p[0], p[2] - p[0])
    d = n @ p[0]
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    want = d / (n[0] * (c - W / 2) / intr[0, 0] + n[1] * (r - H / 2) / intr[1, 1] + n[2])
    err = np.abs(depth.astype(np.float64) - want) / want
    print("tilted quad: max relative error", err.max())
    assert err.max() <= 2.0 ** -24 + 1e-12


@pytest.mark.parametrize("level", [2, 3])
def test_a_vertex_finds_its_own_depth_at_the_pixel_it_queries(level):
    """Every front-facing vertex (camera-space normal z < -0.5) of a sphere passes warp_mesh.py:294-295's visibility test on
    the rendered depth: the pixel int(pix + 0.5) is masked and |lz - depth| < 0.005.  This pins the pixel-centre convention:
    with the principal point half a pixel off the level-2 sphere reaches 0.0058."""
    v, f, extr, intr, pp = ref.sphere_case(level)
    depth, mask, _, _ = ref.render(v, f, ref.cam16(extr, intr, *pp), 96, 128)
    masked, err = ref.consumer_errors(v, extr, intr, pp, depth, mask)
    print(f"icosphere({level}): max |lz - depth| = {err}")
    assert masked and err < 0.005


def test_hand_built_faces():
    v, f, names = ref.hand_built()
    k = {n: i for i, n in enumerate(names)}
    depth, mask, face, n_clipped = ref.render(v, f, ref.IDENTITY_CAM16, ref.HAND_H, ref.HAND_W)
    drawn = set(np.unique(face)) - {-1}
    # two coincident faces: the lower index wins every pixel, at the plane's depth
    assert k["coincident_a"] in drawn and k["coincident_b"] not in drawn
    assert face[12, 12] == k["coincident_a"] and abs(float(depth[12, 12]) - 2.0) < 1e-6
    assert face[10, 10] == face[10, 20] == face[20, 10] == k["coincident_a"]          # corners and edges are inclusive
    assert face[16, 16] == -1 and mask[16, 16] == 0 and depth[16, 16] == np.float32(100.0)
    # zero area, off screen: absent and not counted; behind the near plane: absent and counted
    assert k["zero_area"] not in drawn and k["off_screen"] not in drawn and k["behind"] not in drawn
    assert n_clipped == 1 and (mask[5:15, 88:102] == 0).all()
    # a vertex exactly at a pixel centre is covered, its neighbours along the row and the column are not
    assert face[30, 40] == k["at_centre"] and mask[30, 40] == 255 and abs(float(depth[30, 40]) - 2.0) < 1e-6
    assert face[30, 41] == -1 and face[31, 40] == -1 and face[31, 41] == k["at_centre"]
    # the wedge from 1e10 units away: drawn at the left border only, and symmetric about its axis (row 48)
    assert k["wedge"] in drawn and face[48, 0] == face[48, 5] == k["wedge"] and face[48, 6] == -1
    assert (face[:, 6:] != k["wedge"]).all() and (face[:40] != k["wedge"]).all() and (face[57:] != k["wedge"]).all()
    assert ((mask == 255) == (face >= 0)).all() and ((depth == np.float32(100.0)) == (face < 0)).all()


def test_no_faces_is_the_background():
    depth, mask, face, n_clipped = ref.render(np.zeros((0, 3)), np.zeros((0, 3), np.int64), ref.IDENTITY_CAM16, 5, 7, background=42.0)
    assert depth.shape == (5, 7) and depth.dtype == np.float32 and (depth == np.float32(42.0)).all()
    assert mask.dtype == np.uint8 and not mask.any() and (face == -1).all() and n_clipped == 0


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (96, 128)])
def test_png_gray8_round_trip(tmp_path, shape):
    a = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    path = str(tmp_path / "a.png")
    formats.save_png_gray8(path, a)
    b = formats.load_png_gray8(path)
    assert b.dtype == np.uint8 and np.array_equal(a, b)
    with pytest.raises(ValueError):
        formats.save_png_gray8(path, a.astype(np.float32))


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (96, 128)])
def test_png_gray8_is_read_by_pil_and_reads_pil(tmp_path, shape):
    Image = pytest.importorskip("PIL.Image")
    a = (np.add.outer(np.arange(shape[0]) * 3, np.arange(shape[1]) * 5) % 256).astype(np.uint8)
    path = str(tmp_path / "a.png")
    formats.save_png_gray8(path, a)
    with Image.open(path) as im:
        assert im.mode == "L" and np.array_equal(np.asarray(im), a)
    Image.fromarray(a).save(path, optimize=True)             # (PIL chooses row filters: the reader undoes all five)
    assert np.array_equal(formats.load_png_gray8(path), a)


def test_abi_declares_and_validates_without_gpu(hip_lib):
    from gaustar_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr.h")).read(), flags=re.S)
    for name in ("gsr_mesh_depth_workspace_bytes", "gsr_mesh_depth_view"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SIGNATURES and hasattr(hip_lib, name)
    assert "render_depth_from_mesh.py:13-101" in open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert hip_lib.gsr_abi_version() == 16
    H, W, F = 1080, 1920, 81920
    assert 8 * H * W + 4 * F <= hip_lib.gsr_mesh_depth_workspace_bytes(H, W, F) <= 8 * H * W + 4 * F + 256
    buf = (ctypes.c_double * 64)()                           # host memory: every check below fails before any device work
    p = ctypes.cast(buf, ctypes.c_void_p)
    cam = (ctypes.c_double * 16)(*ref.IDENTITY_CAM16)
    call = lambda **kw: hip_lib.gsr_mesh_depth_view(*[{**dict(H=4, W=4, V=3, F=1, verts=p, faces=p, cam=cam, znear=0.01, bg=100.0,
                                                              small=0, ws=p, depth=p, mask=p, face=None, ncl=p, stream=None), **kw}[k]
                                                      for k in ("H", "W", "V", "F", "verts", "faces", "cam", "znear", "bg", "small",
                                                                "ws", "depth", "mask", "face", "ncl", "stream")])
    for missing in ("verts", "faces", "cam", "ws", "depth", "mask", "ncl"):
        assert call(**{missing: None}) != 0 and b"null" in hip_lib.gsr_last_error(), missing
    assert call(H=0) != 0 and b"positive" in hip_lib.gsr_last_error()
    assert call(W=-3) != 0 and b"positive" in hip_lib.gsr_last_error()
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert call(bg=bad) != 0 and b"background" in hip_lib.gsr_last_error()
    assert call(H=1 << 16, W=1 << 15) != 0 and b"too large" in hip_lib.gsr_last_error()
