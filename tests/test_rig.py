"""gaustar_amd._rig without a GPU: the one layout check of the rig dict against what the two checks it replaced accepted and
rejected, a camera's host blocks against the formulas they were built by (written out here), the principal-point rule, the
npz entry point, and _host.resolve_device's refusal of anything but a GPU before any call into the runtime."""
import ctypes

import numpy as np
import pytest
import torch

from gaustar_amd import _host, _rig, hull, mesh_depth, sweep
from gaustar_amd._rig import Rig

PREP = dict(min_side=1, max_cameras=5)                                 # dataprep's options, with a small limit
HULL = dict(min_side=2, finite=True, positive_focal=True)              # hull's


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _cameras(C=3):
    """Non-trivial rotations, principal points off the centre, an odd width, a shape per camera."""
    intr, extr = np.zeros((C, 3, 3)), np.zeros((C, 4, 4))
    shape = np.array([(6 + i, 9 + 2 * i) for i in range(C)], np.int32)
    for i in range(C):
        extr[i] = np.eye(4)
        extr[i][:3, :3] = _rot((1.0, 0.3 * i - 0.2, 0.7), 0.4 + 0.9 * i)
        extr[i][:3, 3] = (0.1 * i, -0.2, 2.5 + i / 3)
        intr[i] = [[310.5 + i, 0, 4.3 + i], [0, 298.25 - i, 2.9 - i / 7], [0, 0, 1]]
    return {"intrinsics": intr, "extrinsics": extr, "shape": shape}


def test_layout():
    d = _cameras()
    for opts in ({}, PREP, HULL):
        r = Rig.of(d, **opts)
        assert r.C == 3 and r.intr.dtype == r.extr.dtype == np.float64 and r.hw(1) == (7, 11) and Rig.of(r, **HULL) is r
        assert Rig.of(dict(d, extrinsics=d["extrinsics"][:, :3]), **opts).extr.shape == (3, 3, 4)
        assert Rig.of({k: v[:0] for k, v in d.items()}, **opts).C == 0
        for bad in (dict(d, intrinsics=d["intrinsics"][:2]), dict(d, extrinsics=d["extrinsics"][0]), dict(d, extrinsics=d["extrinsics"][:, :2]),
                    dict(d, extrinsics=d["extrinsics"][:, :, :3]), dict(d, shape=d["shape"][:, :1]), dict(d, shape=d["shape"][0]),
                    dict(d, shape=np.zeros(()))):
            with pytest.raises(ValueError, match="rig must hold"):
                Rig.of(bad, **opts)
    assert set(r.as_dict()) == {"intrinsics", "extrinsics", "shape"} and r.as_dict()["shape"] is r.shape


def test_each_caller_keeps_its_own_checks():
    d = _cameras()
    thin = dict(d, shape=np.array([[1, 9], [7, 11], [8, 13]]))
    assert Rig.of(thin, **PREP).hw(0) == (1, 9) and Rig.of(thin).C == 3
    with pytest.raises(ValueError, match="at least 2 x 2"):
        Rig.of(thin, **HULL)
    with pytest.raises(ValueError, match="must be positive"):
        Rig.of(dict(d, shape=np.array([[0, 9], [7, 11], [8, 13]])), **PREP)
    for key, at in (("intrinsics", (1, 0, 2)), ("extrinsics", (2, 1, 3))):
        nan = dict(d, **{key: d[key].copy()})
        nan[key][at] = np.nan
        assert Rig.of(nan, **PREP).C == 3                       # (dataprep never looked)
        with pytest.raises(ValueError, match="finite"):
            Rig.of(nan, **HULL)
    for k in (0, 1):
        flat = dict(d, intrinsics=d["intrinsics"].copy())
        flat["intrinsics"][1, k, k] = 0.0
        assert Rig.of(flat, **PREP).C == 3
        with pytest.raises(ValueError, match="focal"):
            Rig.of(flat, **HULL)
    six = {k: np.concatenate([v, v]) for k, v in d.items()}
    assert Rig.of(six, **HULL).C == 6
    with pytest.raises(ValueError, match="6 cameras: more than 5"):
        Rig.of(six, **PREP)


def _parent_cam14(extr, intr):
    vals = list(np.asarray(extr[:3, :3], np.float64).reshape(-1)) + list(np.asarray(extr[:3, 3], np.float64)) + \
        [float(intr[0, 0]), float(intr[1, 1])]
    return (ctypes.c_double * 14)(*vals)


def _parent_cam16(extr, intr, cx, cy):
    return (ctypes.c_double * 16)(*_parent_cam14(np.asarray(extr), np.asarray(intr)), float(cx), float(cy))


def test_camera_blocks_byte_for_byte():
    d = _cameras()
    r = Rig.of(d)
    for i in range(r.C):
        H, W = (int(x) for x in d["shape"][i])
        e, k = d["extrinsics"][i], d["intrinsics"][i]
        assert bytes(r.cam14(i)) == bytes(_parent_cam14(e, k)) == bytes(sweep.cam14(e, k)) and len(bytes(r.cam14(i))) == 112
        centre, own = _parent_cam16(e, k, W / 2, H / 2), _parent_cam16(e, k, k[0, 2], k[1, 2])
        assert bytes(r.cam16(i)) == bytes(centre) == bytes(mesh_depth.cam16(e, k, W / 2, H / 2)) and bytes(centre) != bytes(own)
        assert bytes(r.cam16(i, True)) == bytes(own) and bytes(r.cam16(i, use_principal_point=True, principal_point=(1.5, 2))) \
            == bytes(_parent_cam16(e, k, 1.5, 2)) == bytes(r.cam16(i, principal_point=(1.5, 2)))
        assert bytes(mesh_depth.cam16(e.tolist(), k.tolist(), 3, 4)) == bytes(_parent_cam16(e, k, 3.0, 4.0))      # (lists, as before)
        # a row of the hull's camera table, filled the way carve_views fills it, against the tuple it was filled by
        for upp, (cx, cy) in ((False, (W / 2, H / 2)), (True, (k[0, 2], k[1, 2]))):
            want, got = np.zeros(1, hull.CAMERA_DTYPE), np.zeros(1, hull.CAMERA_DTYPE)
            want[0] = (e[:3, :3].reshape(-1), e[:3, 3], k[0, 0], k[1, 1], cx, cy, 0x1234, H, W)
            got.view(np.float64).reshape(1, -1)[:, :16] = [r.cam16(i, upp)]
            got["d2"] = [0x1234]
            got["H"], got["W"] = np.array([r.hw(i)]).T
            assert got.tobytes()[:128] == bytes(r.cam16(i, upp)) and got.tobytes() == want.tobytes()
    assert hull.CAMERA_DTYPE.itemsize == 144 and hull.CAMERA_DTYPE.fields["d2"][1] == 128


def test_principal_point_rule():
    r = Rig.of(_cameras())
    assert r.hw(0) == (6, 9) and r.principal(0, False) == (4.5, 3.0) == r.principal(0) == _rig.principal_point(6, 9)
    assert r.principal(0, True) == (4.3, 2.9) and _rig.principal_point(6, 9, (np.float32(1.5), 2)) == (1.5, 2.0)
    assert all(type(x) is float for x in r.principal(0, True) + r.principal(0, False))


@pytest.mark.parametrize("extras", [False, True])
def test_load(tmp_path, extras):
    d = _cameras()
    more = dict(ids=np.arange(10, 13), dist_coeffs=np.arange(15.0).reshape(3, 5)) if extras else {}
    path = tmp_path / "rgb_cameras.npz"
    np.savez(str(path), **d, **more)
    for src in (path, str(path), dict(np.load(str(path))), np.load(str(path))):
        r, info = Rig.load(src, **HULL)
        assert r.C == 3 and all(np.array_equal(getattr(r, a), d[k]) for a, k in (("intr", "intrinsics"), ("extr", "extrinsics"), ("shape", "shape")))
        assert ("ids" in info) == ("dist_coeffs" in info) == extras and (not extras or np.array_equal(info["dist_coeffs"], more["dist_coeffs"]))
    np.savez(str(path), **dict(d, shape=np.ones((3, 2), np.int32)), **more)
    assert Rig.load(path, **PREP)[0].hw(2) == (1, 1)
    with pytest.raises(ValueError, match="at least 2 x 2"):
        Rig.load(path, **HULL)
    with pytest.raises(KeyError):
        Rig.load({"intrinsics": d["intrinsics"], "shape": d["shape"]})


def test_images_checked_on_the_host():
    r = Rig.of({k: v[[0, 0]] for k, v in _cameras().items()})          # two cameras of 6 x 9
    u8, i16 = (torch.uint8,), (torch.uint8, torch.int16)
    stack = np.zeros((2, 6, 9, 3), np.uint8)
    _rig.check_images(stack, r, (3,), u8, "image", stack_only=True)
    _rig.check_images(torch.from_numpy(stack), r, (3,), u8, "image", stack_only=True)         # (dataprep takes a host tensor)
    _rig.check_images(lambda i: None, r, (3,), u8, "image", stack_only=True)
    _rig.check_images([np.zeros((6, 9), np.uint8), np.zeros((6, 9), np.int16)], r, (), i16, "mask", on_gpu=True)
    for bad, kw in ((list(stack), dict(stack_only=True)), (stack[:1], {}), (stack.astype(np.int16), {}), (stack[..., :2], {}), (stack[:, :5], {}),
                    (np.zeros((0, 6, 9, 3), np.float32), dict(stack_only=True)), (np.zeros((2, 6, 9, 3, 1), np.uint8), dict(stack_only=True))):
        with pytest.raises(ValueError):
            _rig.check_images(bad, r, (3,), u8, "image", **kw)
    with pytest.raises(ValueError, match="on a GPU"):
        _rig.check_images([torch.zeros(6, 9, dtype=torch.uint8)] * 2, r, (), i16, "mask", on_gpu=True)
    cpu = torch.device("cpu")
    got = _rig.fetch_image(lambda i: stack[i][::-1], 1, (6, 9), (3,), u8, cpu, "image")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (6, 9, 3) and got.is_contiguous()
    for src, dtypes in ((stack, i16[1:]), (stack[:, :5], u8)):
        with pytest.raises(ValueError, match="image 1 must be"):
            _rig.fetch_image(src, 1, (6, 9), (3,), dtypes, cpu, "image")


@pytest.mark.parametrize("exc", [RuntimeError, ValueError])
def test_resolve_device_wants_a_gpu(monkeypatch, exc):
    def no_call(*_a, **_k):
        raise AssertionError("the runtime was asked")
    monkeypatch.setattr(torch.cuda, "current_device", no_call)
    monkeypatch.setattr(torch._C, "_cuda_getDevice", no_call)
    for device in ("cpu", torch.device("cpu"), "meta"):
        with pytest.raises(exc, match="X needs a GPU"):
            _host.resolve_device(device, torch.zeros(1), what="X", exc=exc)
    assert _host.resolve_device("cuda:1", what="X") == torch.device("cuda", 1)       # an index given is the answer
    assert _host.resolve_device(torch.device("cuda", 0), torch.zeros(1), what="X").index == 0
