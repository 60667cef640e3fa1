"""GPU: the one launch rule of the mesh mirrors (gaustar_amd._host).  Every entry point of include/gsr.h that ends in a
`gsr_stream_t stream` is wrapped by a spy that lets no wrong launch reach the device: when it is called, the tensors' device
must be the current one and the stream argument must be PyTorch's current stream of that device.  Under the spy the public
functions run (a) inside a side stream of the current device and (b), with two GPUs, on the device that is not current; every
result must have the bits of the plain call on the current device's default stream."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import warp_scene as ws
from test_abi import _declared

pytestmark = pytest.mark.gpu
# (gsr_release_stream_state's only parameter names the stream whose state goes; it launches nothing)
STREAM_ENTRY_POINTS = sorted(n for n, (_ret, n_args, args) in _declared().items()
                             if n_args > 1 and args.split(",")[-1].split() == ["gsr_stream_t", "stream"])
N_QUERIES, IMAGE, K, TARGET_FACES, G = 32, 16, 4, 40, 3      # (G: Gaussians per triangle, one of 1, 3, 4, 6)


# ---------------------------------------------------------------------------------------------------- the spy
def _spy(monkeypatch, lib, dev, never_null):
    """-> the list the wrappers append every forwarded launch's name to."""
    seen = []

    def wrap(name, real):
        def launch(*args):
            assert torch.cuda.current_device() == dev.index, f"{name}: the current device is not {dev}"
            st = args[-1]
            st = 0 if st is None else (st.value or 0) if isinstance(st, ctypes.c_void_p) else int(st)
            assert st == torch._C._cuda_getCurrentRawStream(dev.index), f"{name}: not the current stream of {dev}"
            assert st != 0 or not never_null, f"{name}: launched on the default stream"
            seen.append(name)
            return real(*args)
        return launch

    for name in STREAM_ENTRY_POINTS:
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return seen


def _leaves(x):
    """A result as a flat list of host values: tensors on the CPU with floats viewed as integers, floats as their bits."""
    if torch.is_tensor(x):
        x = x.detach().cpu()
        return [x.view({4: torch.int32, 8: torch.int64}[x.element_size()]) if x.is_floating_point() else x]
    if isinstance(x, np.ndarray):
        return _leaves(torch.from_numpy(np.ascontiguousarray(x)))
    if dataclasses.is_dataclass(x):
        return [v for f in dataclasses.fields(x) for v in _leaves(getattr(x, f.name))]
    if isinstance(x, (tuple, list)):
        return [v for y in x for v in _leaves(y)]
    if isinstance(x, float):
        return [int(np.float64(x).view(np.int64))]
    assert x is None or isinstance(x, (bool, int, str)), type(x)
    return [x]


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        if torch.is_tensor(a):
            assert torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
        else:
            assert a == b


# ---------------------------------------------------------------------------------------------------- the inputs
def _sphere():
    from gaustar_amd import scene
    v, f = scene.icosphere(1, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


class Inputs:
    """The smallest inputs that reach every launch, on `dev`: an icosphere of 80 faces (and the same without its last face, so
    there is a rim), 32 query points, 16 x 16 images, two cameras."""

    def __init__(self, dev):
        from gaustar_amd import harness, scene, topology
        self.dev = dev
        rng = np.random.default_rng(7)
        v, f = _sphere()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.V, self.F = len(v), len(f)
        self.verts, self.faces, self.open = up(v), up(f), up(f[:-1])
        self.colors = up(rng.random((self.V, 3)).astype(np.float32))
        self.queries = up((np.asarray(scene.SUBJECT_CENTER) + rng.normal(0, 0.7, (N_QUERIES, 3))).astype(np.float32))
        self.mask = up(np.arange(self.F) % 3 != 0)
        c = np.asarray(scene.SUBJECT_CENTER, np.float64)
        self.box = np.stack([c - [2.0, 0.0, 2.0], c + [2.0, 2.0, 2.0]])           # the upper half of the sphere
        self.sh_dc = up(rng.normal(0, 1.2, (self.F * G, 3)).astype(np.float32))
        self.rgba = up(rng.integers(0, 256, (self.F, 4)).astype(np.uint8))
        self.bary = up(np.array([[0.6, 0.2, 0.2], [0.2, 0.6, 0.2], [0.2, 0.2, 0.6]], np.float32))
        self.origin = up(np.array([0, 5, -1, -1 - (self.F - 1), -2 ** 31, self.F - 1], np.int32))
        self.pred = up(rng.random((3, IMAGE, IMAGE)).astype(np.float32))
        self.gt = up(rng.random((3, IMAGE, IMAGE)).astype(np.float32))
        self.pixels = up(rng.random((IMAGE, IMAGE)) < 0.5)
        self.scaling = up(rng.uniform(0.05, 0.2, (self.V, 3)).astype(np.float32))
        self.quats = up(rng.normal(0, 1, (self.V, 4)).astype(np.float32))
        self.strengths = up(rng.uniform(0.1, 1.0, self.V).astype(np.float32))
        eyes = [(3.0, 1.6, 0.5), (-0.5, 1.0, 3.0)]
        self.cams = [harness.nerf_camera_from_scene(scene.look_at_camera(e, scene.SUBJECT_CENTER, IMAGE, IMAGE, focal_px=12.0))
                     for e in eyes]
        self.rig = topology.rig_from_cameras(self.cams)
        self.frames = [ws.frames(self.rig["extrinsics"][i], self.rig["intrinsics"][i], self.rig["shape"][i], scene.SUBJECT_CENTER,
                                 scene.SUBJECT_RADIUS, dev) for i in range(2)]
        self.depth = up(np.full((IMAGE, IMAGE), 1.0, np.float32))
        self.rgb8 = up(rng.integers(0, 256, (IMAGE, IMAGE, 3)).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------- the calls
def _regions(x):
    from gaustar_amd import regions as r
    cut = r.cut_mesh_by_box(x.verts, x.faces, x.box, False, attrs=(x.colors,))
    base = r.cut_mesh_by_box(x.verts, x.faces, x.box, True)
    b_cut, b_base = r.boundary_vertices(cut.verts, cut.faces), r.boundary_vertices(base.verts, base.faces)
    return [r.face_edge_counts(x.open, x.mask[:-1]), r.face_components(x.faces, x.mask), cut, base, b_cut, b_base,
            r.boundary_vertices(x.verts, x.open), r.boundary_vertices(base.verts, base.faces, x.box, True),
            r.boundary_vertices(cut.verts, cut.faces, x.box, False), r.outlier_component_mask(x.open),
            r.nearest_vertices(x.queries, x.verts, return_max=True), r.select_faces(x.verts, x.faces, x.mask, attrs=(x.colors,)),
            r.is_watertight(x.faces), r.is_watertight(x.open), r.fill_small_holes(x.open, x.V), r.face_areas(x.verts, x.faces),
            r.mean_edge_length(x.verts, x.faces), r.merge_vertices_around_holes(x.verts, x.open),
            r.compose_face_mask(x.mask, x.mask[:int(x.mask.sum())]),
            r.connect_two_meshes(base.verts, base.faces, b_base, cut.verts, cut.faces, b_cut)]


def _handover(x):
    from gaustar_amd import handover as h
    return [h.sh_face_colors(x.sh_dc, G), h.vertex_to_face_colors(x.faces, x.colors), h.face_to_vertex_colors(x.faces, x.rgba, x.V),
            h.sh_dc_from_vertex_colors(x.faces, x.colors, x.bary), h.gather_face_colors(x.origin, x.rgba, x.faces, x.colors)]


def _tracking(x):
    from gaustar_amd import tracking
    tracker = tracking.SurfaceTracker.dense(x.F, device=x.dev)
    pos = tracker.positions(x.verts, x.faces)
    survive = torch.ones(x.F, dtype=torch.bool, device=x.dev)
    survive[-1] = False
    stats = tracker.rebind(pos, survive, x.verts * 1.01, x.open)
    return [pos, tuple(stats), tracker.face_ids, tracker.face_bary, tracking.bind_points(x.verts, x.faces, x.queries.double())]


def _evaluate(x):
    from gaustar_amd import evaluate as e
    mesh, other = (x.verts.double(), x.faces), (x.verts.double() * 1.02, x.open)
    md = e.mesh_distance(mesh, other, n_samples=N_QUERIES, return_samples=True)
    return [tuple(e.surface_distance(x.queries.double(), *mesh)), tuple(e.sample_surface(*mesh, N_QUERIES, seed=3)),
            [md[0].a_to_b, md[0].b_to_a, md[0].chamfer, md[0].fscore, tuple(md[1]), tuple(md[2])],
            tuple(e.image_metrics(x.pred, x.gt)), tuple(e.image_metrics(x.pred, x.gt, mask=x.pixels, clamp=False))]


def _remesh(x):
    from gaustar_amd import remesh
    small = remesh.simplify_mesh(x.verts, x.faces, TARGET_FACES, attrs=(x.colors,))
    assert small.n_rounds > 0
    return [small, remesh.smooth_taubin(x.verts, x.faces, iterations=2)]


def _knn(x):
    from gaustar_amd import knn
    return [knn.nearest_neighbors(x.queries, x.verts, K=K), knn.dist_cuda2(x.verts)]


def _density(x):
    from gaustar_amd import density, knn
    idx = knn.nearest_neighbors(x.queries, x.verts, K=K)[0]
    args = (x.queries, x.verts, x.scaling, x.quats, x.strengths)
    return [density.compute_density(*args, K=K), density.compute_density(*args, closest_gaussians_idx=idx, return_closest_gaussian_opacities=True)]


def _mesh_depth(x):
    from gaustar_amd import mesh_depth
    views = []

    def sink(i, view):
        views.append((i, view.depth.clone(), view.mask.clone()))
    one = mesh_depth.mesh_depth_view(x.verts, x.faces, x.rig["extrinsics"][0], x.rig["intrinsics"][0], IMAGE, IMAGE, return_faces=True)
    assert int(one.mask.sum()) > 0
    mesh_depth.render_mesh_depth(x.verts, x.faces, x.rig, sink, views_in_flight=1)
    return [one, views]


def _fusion(x):
    from gaustar_amd import fusion
    vol = fusion.TSDFVolume([-0.05] * 3, [0.05] * 3, 0.02, 0.05, x.dev)
    extr = np.eye(4)
    extr[2, 3] = 1.0                                       # the camera one unit in front of the plane z = 0
    fusion.integrate_views(vol, x.depth, x.rgb8, (16.0, 16.0, IMAGE / 2, IMAGE / 2), extr)
    mesh = fusion.extract_triangle_mesh(vol)
    assert mesh[1].shape[0] > 0
    depth_alpha = torch.stack([x.pred[0] * 3, x.pred[1], x.pred[2]])
    return [vol.tsdf, vol.weight, vol.color, mesh, fusion.prepare_images(x.gt, depth_alpha)]


def _warp(x):
    from gaustar_amd import warp
    cfg = warp.WarpConfig(edge_scalar=100, min_observe=1)
    res = warp.warp_mesh(x.verts.double(), x.faces.long(), x.rig, lambda i: x.frames[i], cfg, return_stages=True)
    return [res.table, res.normals, res.move_raw, res.move_propagated, res.move_smoothed, res.observed, res.count]


def _topology(x):
    from gaustar_amd import harness, topology
    model = harness.SurfaceGaussians(x.verts, x.faces.long(), n_gaussians_per_surface_triangle=G, sh_levels=1)
    renders = topology.DepthRenders(model)
    gt = torch.stack([renders(c)[0] for c in x.cams]) * 1.05
    res = topology.detect_topology_errors(model, x.cams, gt, min_observe=1, return_stages=True)
    return [res.table, res.count, res.value, res.propagated, res.interpolated, res.face_loss, res.face_colour, res.topo_change_num]


CALLS = {"regions": _regions, "handover": _handover, "tracking": _tracking, "evaluate": _evaluate, "remesh": _remesh, "knn": _knn,
         "density": _density, "mesh_depth": _mesh_depth, "fusion": _fusion, "warp": _warp, "topology": _topology}
_plain = {}


def _reference(feature):
    """The plain call on the current device's default stream, once per feature."""
    if feature not in _plain:
        dev = torch.device("cuda", torch.cuda.current_device())
        _plain[feature] = _leaves(CALLS[feature](Inputs(dev)))
        torch.cuda.synchronize(dev)
    return _plain[feature]


@pytest.mark.parametrize("feature", sorted(CALLS))
def test_on_a_side_stream(hip_lib, monkeypatch, feature):
    want = _reference(feature)
    dev = torch.device("cuda", torch.cuda.current_device())
    side = torch.cuda.Stream(dev)
    assert side.cuda_stream != 0
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        x = Inputs(dev)
        seen = _spy(monkeypatch, hip_lib, dev, never_null=True)
        got = _leaves(CALLS[feature](x))
    side.synchronize()
    assert seen, "the spy saw no launch"
    _same(got, want)


@pytest.mark.parametrize("feature", sorted(CALLS))
def test_on_the_device_that_is_not_current(hip_lib, monkeypatch, feature):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: every tensor lives on the device that is not current")
    want = _reference(feature)
    here = torch.cuda.current_device()
    dev = torch.device("cuda", 1 if here == 0 else 0)
    x = Inputs(dev)
    seen = _spy(monkeypatch, hip_lib, dev, never_null=False)
    got = _leaves(CALLS[feature](x))
    torch.cuda.synchronize(dev)
    assert seen, "the spy saw no launch"
    assert torch.cuda.current_device() == here
    _same(got, want)
