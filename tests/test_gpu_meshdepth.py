"""The mesh depth rasterizer on the device (gsr_meshdepth.hip behind gaustar_amd.mesh_depth) against its numpy restatement
tests/meshdepth_ref.py, bit for bit, on 128 x 96 and 67 x 45 images."""
import os

import numpy as np
import pytest
import torch

import meshdepth_ref as ref
from gaustar_amd import formats, harness, mesh_depth, scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _split(cam):
    """cam16 -> (extr [4,4], intr [3,3], (cx, cy))."""
    extr = np.eye(4)
    extr[:3, :3], extr[:3, 3] = cam[:9].reshape(3, 3), cam[9:12]
    return extr, np.array([[cam[12], 0, cam[14]], [0, cam[13], cam[15]], [0, 0, 1.0]]), (cam[14], cam[15])


def _np(view):
    return (view.depth.cpu().numpy(), view.mask.cpu().numpy(), None if view.face is None else view.face.cpu().numpy(),
            int(view.n_clipped.cpu()))


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


@pytest.fixture(scope="module")
def combined():
    """The mesh, the three cameras and the restatement's images, computed once."""
    verts, faces = ref.combined_mesh()
    cams = ref.combined_cameras()
    want = [ref.render(verts, faces, cam, H, W) for cam, H, W in cams]
    return verts, faces, cams, want


def _render(verts, faces, cam, H, W, **kw):
    extr, intr, pp = _split(cam)
    return mesh_depth.mesh_depth_view(verts, faces, extr, intr, H, W, principal_point=pp, return_faces=True, **kw)


def test_bits_equal_the_restatement(combined):
    verts, faces, cams, want = combined
    # the scene does what it is for: the big triangle and the sphere are both seen, something is clipped
    big = int(np.nonzero((faces == np.arange(3) + 642).all(1))[0][0])
    assert (want[0][2] == big).sum() > 96 * 128 // 2 and (want[0][2] < big).sum() > 1000 and want[0][3] == 1
    assert all((w[2] == big).any() and (w[2] < big).any() for w in want)
    for (cam, H, W), w in zip(cams, want):
        got = _np(_render(verts, faces, cam, H, W))
        assert got[0].dtype == np.float32 and got[1].dtype == np.uint8 and got[2].dtype == np.int32 and got[0].shape == (H, W)
        assert got[3] == w[3]
        assert np.array_equal(got[2], w[2]) and np.array_equal(got[1], w[1])
        assert got[0].view(np.uint32).tobytes() == w[0].view(np.uint32).tobytes()


@pytest.mark.parametrize("small_max", [1, 10 ** 9])
def test_result_does_not_depend_on_small_max(combined, small_max):
    """small_max = 1 sends every face of more than one pixel through the big-face pass, 10^9 walks even the triangle over the
    whole image in one lane: both equal the restatement, as the default does, which mixes the two."""
    verts, faces, cams, want = combined
    for (cam, H, W), w in zip(cams, want):
        assert _same(_np(_render(verts, faces, cam, H, W, small_max=small_max)), w)


def test_reproducible_and_independent_of_views_in_flight(combined):
    verts, faces, cams, want = combined
    cam, H, W = cams[0]
    assert _same(_np(_render(verts, faces, cam, H, W)), _np(_render(verts, faces, cam, H, W)))
    rig = {"extrinsics": np.stack([_split(c)[0] for c, _, _ in cams]), "intrinsics": np.stack([_split(c)[1] for c, _, _ in cams]),
           "shape": np.array([[H, W] for _, H, W in cams])}
    runs = []
    for vif in (1, 2):
        got = {}
        done = mesh_depth.render_mesh_depth(verts, faces, rig, lambda i, view: got.__setitem__(i, view), use_principal_point=True,
                                            views_in_flight=vif, return_faces=True)
        assert done == [0, 1, 2] and sorted(got) == [0, 1, 2]
        runs.append([_np(got[i]) for i in range(3)])
    for i in range(3):
        assert _same(runs[0][i], runs[1][i]) and _same(runs[0][i], want[i])
    # a shard renders its own cameras only, and without the principal point the centre of the image is used
    got = {}
    assert mesh_depth.render_mesh_depth(verts, faces, rig, lambda i, view: got.__setitem__(i, view), rank=1, world=2,
                                        views_in_flight=1) == [1]
    cam, H, W = cams[1]
    cam = cam.copy()
    cam[14:16] = W / 2, H / 2
    centred = ref.render(verts, faces, cam, H, W)
    assert sorted(got) == [1] and got[1].face is None and got[1].depth.cpu().numpy().tobytes() == centred[0].tobytes()


def test_out_buffers_no_faces_and_odd_alignment():
    """`out` is written in place; F == 0 yields the background; a view whose outputs are not 16-byte aligned (the resolve
    kernel's one-pixel path) equals the aligned one."""
    verts, faces = ref.combined_mesh()
    cam, H, W = ref.combined_cameras()[2]
    extr, intr, pp = _split(cam)
    a = _render(verts, faces, cam, H, W)
    pool = [torch.zeros(H * W + 1, dtype=dt, device=DEV)[1:].view(H, W) for dt in (torch.float32, torch.uint8, torch.int32)]
    out = mesh_depth.MeshDepthView(pool[0], pool[1], pool[2], torch.zeros(1, dtype=torch.int32, device=DEV))
    b = mesh_depth.mesh_depth_view(verts, faces, extr, intr, H, W, principal_point=pp, return_faces=True, out=out)
    assert b.depth.data_ptr() == pool[0].data_ptr() and b.depth.data_ptr() % 16 != 0 and _same(_np(a), _np(b))
    e = mesh_depth.mesh_depth_view(np.zeros((0, 3)), np.zeros((0, 3), np.int64), extr, intr, 45, 67, background=7.5, return_faces=True)
    d, m, f, n = _np(e)
    assert (d == np.float32(7.5)).all() and not m.any() and (f == -1).all() and n == 0
    with pytest.raises(ValueError):
        mesh_depth.mesh_depth_view(verts, faces, extr, intr, H, W, out=mesh_depth.MeshDepthView(pool[0], pool[2], None, out.n_clipped))


@pytest.mark.parametrize("level", [2, 3])
def test_a_vertex_finds_its_own_depth_on_the_device(level):
    v, f, extr, intr, pp = ref.sphere_case(level)
    view = mesh_depth.mesh_depth_view(v, f, extr, intr, 96, 128)
    masked, err = ref.consumer_errors(v, extr, intr, pp, view.depth.cpu().numpy(), view.mask.cpu().numpy())
    print(f"icosphere({level}) on the device: max |lz - depth| = {err}")
    assert masked and err < 0.005


def test_files_follow_the_reference_layout(tmp_path):
    v, f = scene.icosphere(1, 120.0)                          # (millimetres: the folder branch scales by 0.001)
    v = np.asarray(v, np.float64)
    meshes = tmp_path / "meshes"
    meshes.mkdir()
    formats.save_obj(str(meshes / "scan_000.obj"), v, f)
    formats.save_obj(str(meshes / "scan_001.obj"), v * 0.9, f)
    shapes = np.array([[96, 128], [45, 67], [50, 70]])
    cams = [scene.look_at_camera(eye, (0.0, 0.0, 0.0), int(w), int(h), focal_px=300.0)
            for eye, (h, w) in zip(((0.4, -0.3, 3.0), (-2.0, 0.5, 1.5), (0.1, 2.5, -1.0)), shapes)]
    extr = np.stack([ref.camera_of(c)[0] for c in cams])
    intr = np.stack([ref.camera_of(c)[1] for c in cams])
    intr[1, 0, 2] += 3.25                                     # one principal point off the centre
    np.savez(str(tmp_path / "rgb_cameras.npz"), ids=np.arange(3), intrinsics=intr, extrinsics=extr, shape=shapes)
    out = tmp_path / "work"
    mesh_depth.render_mesh_depth_files(str(tmp_path / "rgb_cameras.npz"), meshes, out, frame_0=4)
    want = sorted([f"{i:04d}/depth/img_{c:04d}_depth.npz" for i in (4, 5) for c in range(3)] +
                  [f"{i:04d}/masks/img_{c:04d}_alpha.png" for i in (4, 5) for c in range(3)])
    have = sorted(os.path.relpath(os.path.join(d, n), str(out)) for d, _, names in os.walk(str(out)) for n in names)
    assert have == want
    for i, s in ((4, 1.0), (5, 0.9)):
        for c in range(3):
            with np.load(str(out / f"{i:04d}/depth/img_{c:04d}_depth.npz")) as z:
                assert list(z.keys()) == ["depth"]
                depth = z["depth"]
            assert depth.dtype == np.float32 and depth.shape == tuple(shapes[c])
            mask = formats.load_png_gray8(str(out / f"{i:04d}/masks/img_{c:04d}_alpha.png"))
            assert np.array_equal(mask, np.where(depth < np.float32(100.0), 255, 0).astype(np.uint8)) and mask.any() and not mask.all()
            cam = ref.cam16(extr[c], intr[c], intr[c, 0, 2], intr[c, 1, 2])
            assert depth.tobytes() == ref.render(v * s * 0.001, f, cam, *shapes[c])[0].tobytes()
    (meshes / "scan_002.ply").write_text("ply\n")
    with pytest.raises(ValueError):
        mesh_depth.render_mesh_depth_files(str(tmp_path / "rgb_cameras.npz"), meshes, out)


def test_model_renders_its_own_mesh():
    v, f = scene.icosphere(2, 0.12)
    model = harness.SurfaceGaussians(torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).long().to(DEV), sh_levels=1)
    cams = [harness.nerf_camera_from_scene(scene.look_at_camera(eye, (0.0, 0.0, 0.0), 67, 45, focal_px=400.0))
            for eye in ((0.4, -0.3, 3.0), (-2.0, 0.5, 1.5))]
    from gaustar_amd import topology
    rig = topology.rig_from_cameras(cams)
    for i in range(2):
        a = model.render_mesh_depth(i, cams, return_faces=True)
        b = model.render_mesh_depth(cams[i], return_faces=True)
        c = mesh_depth.mesh_depth_view(model._points.detach(), model._surface_mesh_faces, rig["extrinsics"][i], rig["intrinsics"][i],
                                       45, 67, return_faces=True)
        assert _same(_np(a), _np(c)) and _same(_np(b), _np(c)) and a.mask.any() and not a.mask.all()
