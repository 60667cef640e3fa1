"""The data-preparation kernels on the device (gsr_prep.hip behind gaustar_amd.dataprep) against their numpy restatement
tests/prep_ref.py, bit for bit: rectified images of 45 x 67 x 3 and 96 x 128 x {1, 4}, the vertex colours of a 642-vertex
sphere from six and from three cameras of 128 x 96."""
import os

import numpy as np
import pytest
import torch

import prep_ref as ref
from gaustar_amd import dataprep, formats, harness

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SIZES = [(45, 67, 3), (96, 128, 1), (96, 128, 4)]              # none is a multiple of a wave in width
BORDER = (7, 200, 33, 129)
DIST = (-0.2, 0.05, 1e-3, -2e-3, 0.01)
PATHS = {"fractional": ((3.25, -2.5), None, None), "integer": ((5.0, -3.0), None, None), "outside": ((None, 4.0), None, None),
         "zero_dist": ((3.25, -2.5), (0.0,) * 5, None), "distorted": ((3.25, -2.5), DIST, 60.0)}


def _source(h, w, c):
    return ref.hash_image(h + c, h, w, c)


def _case(h, w, c, path):
    (dx, dy), dist, focal = PATHS[path]
    dx = w + 10.5 if dx is None else dx                         # "outside": a shift larger than the image
    f = 500.0 if focal is None else focal
    intr = np.array([[f, 0.0, w / 2 + dx], [0.0, f, h / 2 + dy], [0.0, 0.0, 1.0]])
    return intr, dist, (f, f, w / 2 + dx, h / 2 + dy)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_rectify_equals_the_restatement(size, path):
    h, w, c = size
    src = _source(h, w, c)
    intr, dist, cam4 = _case(h, w, c, path)
    want = ref.rectify(src, cam4, dist, BORDER[:c])
    got = dataprep.rectify_image(src, intr, dist, BORDER[:c])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, c) and got.is_cuda
    diff = np.nonzero(got.cpu().numpy() != want)
    print(f"{size} {path}: {len(diff[0])} bytes differ")
    assert len(diff[0]) == 0
    if path == "outside":
        assert (want == np.asarray(BORDER[:c], np.uint8)).all()
    elif path == "distorted":
        assert (want != ref.rectify(src, cam4, None, BORDER[:c])).mean() > 0.5      # the distortion moves the image
    else:
        assert (want == np.asarray(BORDER[:c], np.uint8)).all(-1).any() and not (want == np.asarray(BORDER[:c], np.uint8)).all()


def test_rectify_of_a_2d_image_and_a_scalar_border():
    src = _source(96, 128, 1)[:, :, 0]
    intr, dist, cam4 = _case(96, 128, 1, "distorted")
    got = dataprep.rectify_image(torch.from_numpy(src).to(DEV), intr, dist, 77)
    assert tuple(got.shape) == (96, 128) and np.array_equal(got.cpu().numpy(), ref.rectify(src, cam4, dist, 77))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("path", ["fractional", "distorted"])
def test_rectify_one_byte_off_alignment_and_out(size, path):
    """src and dst one byte past a 16-byte boundary (the byte-store path) equal the aligned run (whole dwords); `out` is
    written in place."""
    h, w, c = size
    src = _source(h, w, c)
    intr, dist, cam4 = _case(h, w, c, path)
    aligned_src = torch.from_numpy(src).to(DEV)
    aligned_out = torch.zeros(h, w, c, dtype=torch.uint8, device=DEV)
    assert aligned_src.data_ptr() % 16 == 0 and aligned_out.data_ptr() % 16 == 0
    a = dataprep.rectify_image(aligned_src, intr, dist, BORDER[:c], out=aligned_out)
    assert a.data_ptr() == aligned_out.data_ptr()
    n = h * w * c
    pool_src, pool_out = torch.zeros(n + 1, dtype=torch.uint8, device=DEV), torch.zeros(n + 1, dtype=torch.uint8, device=DEV)
    off_src, off_out = pool_src[1:].view(h, w, c), pool_out[1:].view(h, w, c)
    off_src.copy_(aligned_src)
    assert off_src.data_ptr() % 16 == 1 and off_out.data_ptr() % 16 == 1
    b = dataprep.rectify_image(off_src, intr, dist, BORDER[:c], out=off_out)
    assert b.data_ptr() == off_out.data_ptr() and int(pool_out[0]) == 0
    want = ref.rectify(src, cam4, dist, BORDER[:c])
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want)
    with pytest.raises(ValueError):
        dataprep.rectify_image(aligned_src, intr, dist, BORDER[:c], out=aligned_src)
    with pytest.raises(ValueError):
        dataprep.rectify_image(aligned_src, intr, dist, BORDER[:c], out=aligned_out[:-1])


# ---------------------------------------------------------------------------------------------- colours
@pytest.fixture(scope="module")
def full():
    return ref.rig_case(ref.FULL_RIG_ANGLES)


@pytest.fixture(scope="module")
def half():
    return ref.rig_case(ref.HALF_RIG_ANGLES)


def _same_colors(cols: dataprep.MeshColors, want: dict) -> None:
    assert cols.rgb.dtype == torch.uint8 and cols.filled_at.dtype == torch.uint8 and cols.count.dtype == torch.int32
    assert cols.mean.dtype == torch.float64 and cols.mean.cpu().numpy().view(np.uint64).tolist() == want["mean"].view(np.uint64).tolist()
    assert np.array_equal(cols.rgb.cpu().numpy(), want["rgb"])
    assert np.array_equal(cols.count.cpu().numpy(), want["count"])
    assert np.array_equal(cols.filled_at.cpu().numpy(), want["filled_at"])
    assert (cols.n_unseen, cols.n_unfilled) == (want["n_unseen"], want["n_unfilled"])


def test_colors_full_rig(full):
    n = full["sums"][:, 3]
    assert len(n) == 642 and n.min() >= 1 and n.max() <= 4          # every vertex is seen, by 1 to 4 cameras
    sums = dataprep.view_color_sums(full["verts"], full["rig"], full["images"], faces=full["faces"])      # depths rendered here
    assert sums.dtype == torch.int32 and np.array_equal(sums.cpu().numpy(), full["sums"])
    want = ref.finish(full["sums"], full["neighbours"], 8)
    cols = dataprep.color_mesh_from_views(full["verts"], full["faces"], full["rig"], full["images"])
    _same_colors(cols, want)
    assert cols.n_unseen == 0 and not bool(cols.filled_at.any())
    # the depth maps handed in (the restatement's, pinned bit for bit to the kernel's) and a callable give the same sums
    given = dataprep.view_color_sums(full["verts"], full["rig"], lambda i: full["images"][i], torch.from_numpy(full["depths"]).to(DEV))
    assert torch.equal(given, sums)


def test_colors_half_rig(half):
    seen = (half["sums"][:, 3] > 0).mean()
    assert 0.5 <= seen <= 0.8
    assert ref.finish(half["sums"], half["neighbours"], 3)["n_unfilled"] > 0
    assert ref.finish(half["sums"], half["neighbours"], 7)["n_unfilled"] == 0
    sums = dataprep.view_color_sums(half["verts"], half["rig"], half["images"], faces=half["faces"])
    assert np.array_equal(sums.cpu().numpy(), half["sums"])
    faces = torch.from_numpy(half["faces"]).to(DEV)
    for sweeps in (0, 3, 8):
        want = ref.finish(half["sums"], half["neighbours"], sweeps, (10, 20, 30))
        cols = dataprep.finish_colors(sums, faces if sweeps else None, sweeps, (10, 20, 30))
        _same_colors(cols, want)
        left = cols.filled_at.cpu().numpy() == 255
        assert left.sum() == want["n_unfilled"] and (cols.rgb.cpu().numpy()[left] == (10, 20, 30)).all()
    zero = dataprep.finish_colors(sums, None, 0)
    assert zero.n_unfilled == zero.n_unseen == 222 and bool(torch.isnan(zero.mean[zero.count == 0]).all())


def test_colors_do_not_depend_on_views_in_flight_or_sharding(full):
    args = (full["verts"], full["rig"], full["images"])
    one = dataprep.view_color_sums(*args, faces=full["faces"], views_in_flight=1)
    two = dataprep.view_color_sums(*args, faces=full["faces"], views_in_flight=2)
    assert torch.equal(one, two) and np.array_equal(one.cpu().numpy(), full["sums"])
    r0 = dataprep.view_color_sums(*args, faces=full["faces"], rank=0, world=2)
    r1 = dataprep.view_color_sums(*args, faces=full["faces"], rank=1, world=2)
    assert np.array_equal(r0.cpu().numpy(), full["per_view"][0::2].sum(0)) and np.array_equal(r1.cpu().numpy(), full["per_view"][1::2].sum(0))
    assert torch.equal(r0 + r1, one)


def test_round_trip_into_a_model(tmp_path, half):
    cols = dataprep.color_mesh_from_views(half["verts"], half["faces"], half["rig"], half["images"], fill_sweeps=8)
    assert cols.n_unfilled == 0
    path = str(tmp_path / "init_mesh_100k.obj")
    dataprep.save_init_mesh(path, half["verts"], half["faces"], cols.rgb)
    v, f, c = formats.load_obj(path)
    assert c is not None and c.shape == (642, 3)
    with pytest.raises(ValueError):
        harness.SurfaceGaussians.from_mesh(v, f, None)             # what a mesh without colours gives
    model = harness.SurfaceGaussians.from_mesh(v, f, c, sh_levels=1)
    assert int(model._sh_coordinates_dc.shape[0]) == len(f) * model.n_gaussians_per_surface_triangle
    assert bool(torch.isfinite(model._sh_coordinates_dc).all())
    back = np.clip(np.rint(255.0 * c.astype(np.float32)), 0, 255).astype(np.uint8)     # handover's clip(rint(255 c)) in f32
    assert np.array_equal(back, cols.rgb.cpu().numpy())


def test_launches_follow_the_launch_rule(half):
    """On a side stream every entry point is called with that stream, and the results keep their bits."""
    from gaustar_amd import _lib
    lib = _lib.load()
    names = ("gsr_image_rectify", "gsr_mesh_color_view", "gsr_mesh_color_finish", "gsr_mesh_depth_view")
    real = {n: getattr(lib, n) for n in names}
    plain = dataprep.color_mesh_from_views(half["verts"], half["faces"], half["rig"], half["images"], views_in_flight=1)
    src = _source(45, 67, 3)
    intr, dist, _ = _case(45, 67, 3, "distorted")
    plain_img = dataprep.rectify_image(src, intr, dist)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    seen = []

    def wrap(name):
        def launch(*args):
            st = args[-1]
            st = 0 if st is None else int(st)
            assert st == side.cuda_stream and st != 0, f"{name}: not the current stream"
            seen.append(name)
            return real[name](*args)
        return launch
    try:
        for n in names:
            setattr(lib, n, wrap(n))
        with torch.cuda.stream(side):
            cols = dataprep.color_mesh_from_views(half["verts"], half["faces"], half["rig"], half["images"], views_in_flight=1)
            img = dataprep.rectify_image(src, intr, dist)
        side.synchronize()
    finally:
        for n in names:
            setattr(lib, n, real[n])
    assert set(seen) == set(names)
    assert torch.equal(cols.rgb, plain.rgb) and torch.equal(cols.filled_at, plain.filled_at) and torch.equal(img, plain_img)


def test_first_frame_files(tmp_path):
    """prepare_first_frame on PNG sources: the reference's folders, rectified images equal to the restatement's, the init mesh
    and the COLMAP files of the colours it returns."""
    from gaustar_amd import scene
    v, f = scene.icosphere(2, 0.12)
    v = np.asarray(v, np.float64)
    meshes, source, out = tmp_path / "meshes", tmp_path / "ahq", tmp_path / "gstar"
    meshes.mkdir()
    out.mkdir()
    formats.save_obj(str(meshes / "mesh_000003_smooth_100k.obj"), v, f)
    rig = ref.rig_of((0, 120, 240))
    intr = rig["intrinsics"].copy()
    intr[:, 0, 2] += (3.25, 0.0, -4.0)                            # principal points off the centre
    intr[:, 1, 2] += (-2.5, 1.0, 0.0)
    dist = np.zeros((3, 5))
    dist[2] = (-0.05, 0.01, 1e-4, -2e-4, 0.0)
    np.savez(str(out / "rgb_cameras.npz"), ids=np.arange(1, 4), intrinsics=intr, extrinsics=rig["extrinsics"], shape=rig["shape"],
             dist_coeffs=dist)
    raw = [ref.hash_image(10 + c, ref.H, ref.W) for c in range(3)]
    for c in range(3):
        os.makedirs(str(source / "rgbs" / f"Cam{c + 1:03d}"))
        formats.save_png_rgb8(str(source / "rgbs" / f"Cam{c + 1:03d}" / f"Cam{c + 1:03d}_rgb000003.png"), raw[c])
    cols = dataprep.prepare_first_frame(source, meshes, out, frame_0=3, frame_end=4, fill_sweeps=8)
    have = sorted(os.path.relpath(os.path.join(d, n), str(out)) for d, _, names in os.walk(str(out)) for n in names)
    want = sorted(["rgb_cameras.npz", "init_mesh_100k.obj"] + [f"0003/images/img_{c:04d}.png" for c in range(3)] +
                  [f"0003/depth_humanrf/img_{c:04d}_depth.npz" for c in range(3)] +
                  [f"0003/masks_humanrf/img_{c:04d}_alpha.png" for c in range(3)] +
                  [f"0003/sparse/0/{n}" for n in ("cameras.txt", "images.txt", "points3D.ply")])
    assert have == want
    rect = []
    for c in range(3):
        rect.append(formats.load_png_rgb8(str(out / f"0003/images/img_{c:04d}.png")))
        cam4 = (intr[c, 0, 0], intr[c, 1, 1], intr[c, 0, 2], intr[c, 1, 2])
        assert np.array_equal(rect[c], ref.rectify(raw[c], cam4, dist[c], 0))
    again = dataprep.color_mesh_from_views(v, f, rig, np.stack(rect), fill_sweeps=8)
    assert torch.equal(again.rgb, cols.rgb) and cols.n_unfilled == 0 and 0 < cols.n_unseen < len(v)
    _, _, c = formats.load_obj(str(out / "init_mesh_100k.obj"))
    assert np.array_equal(np.rint(255.0 * c).astype(np.uint8), cols.rgb.cpu().numpy())
    ply = (out / "0003/sparse/0/points3D.ply").read_bytes()
    assert ply.endswith(np.concatenate([v[-1].astype("<f4").view(np.uint8), np.zeros(12, np.uint8), cols.rgb[-1].cpu().numpy()]).tobytes())
