"""gaustar_amd._meshargs: the one decoder of the mesh kernels' err word against a table written out from the four decoders it
replaced (one each in regions, tracking, evaluate and density), and the shared checks of a mesh argument on CPU tensors and
wrong shapes / dtypes.  No GPU."""
import pytest
import torch

from gaustar_amd import _meshargs as ma

IDX = "a vertex index, or another index into the mesh, lies outside its array"
DUP = "a boundary list names a vertex twice"
BOX = "a vertex or Gaussian centre of a kept region is NaN: its box is not defined"
BND = "a boundary position is NaN or infinite: its nearest vertex is not defined"
T_NAN = "a vertex or a tracked position is NaN or infinite"
T_DEG = "a re-bound barycentric is not >= 0: the nearest face of a point is degenerate"
E_IDX = "a vertex index, or another index into the mesh or the points, lies outside its array"
E_NAN = "a vertex or a query point is NaN or infinite, or too large for its distance to be formed: no face is closest"
E_AREA = "no face of the mesh has a positive, finite area (of at least 2^-991): it cannot be sampled"
D_IDX = "compute_density: closest_gaussians_idx holds an index outside [-1, number of Gaussians)"
OK = None      # no raise

# word:            0    1    2      3    4     5    6      7    8       9      10      11     12      13     14      15
TABLE = {
    "regions":   [OK, IDX, BOX,   IDX, DUP,  IDX, DUP,   IDX, OK,     IDX,   BOX,    IDX,   DUP,    IDX,   DUP,    IDX],
    "boundary":  [OK, IDX, BND,   IDX, DUP,  IDX, DUP,   IDX, OK,     IDX,   BND,    IDX,   DUP,    IDX,   DUP,    IDX],
    "handover":  [OK, IDX, BOX,   IDX, DUP,  IDX, DUP,   IDX, OK,     IDX,   BOX,    IDX,   DUP,    IDX,   DUP,    IDX],
    "tracking":  [OK, IDX, T_NAN, IDX, DUP,  IDX, DUP,   IDX, T_DEG,  IDX,   T_NAN,  IDX,   DUP,    IDX,   DUP,    IDX],
    "evaluate":  [OK, E_IDX, E_NAN, E_IDX, OK, E_IDX, E_NAN, E_IDX, E_AREA, E_IDX, E_AREA, E_IDX, E_AREA, E_IDX, E_AREA, E_IDX],
    "density":   [OK, D_IDX, OK, D_IDX, OK, D_IDX, OK,   D_IDX, OK,   D_IDX, OK,     D_IDX, OK,     D_IDX, OK,     D_IDX],
}


def _decoders():
    """Each user's call of the one decoder, with the arguments its module passes."""
    from gaustar_amd import density, evaluate, handover, regions, remesh, tracking
    for module in (regions, handover, remesh, tracking, evaluate, density):
        assert module._ma is ma and not hasattr(module, "_raise_if")        # (no decoder of its own any more)
    return {"regions": lambda w: ma.raise_if(w),
            "boundary": lambda w: ma.raise_if(w, ma.NAN_BOUNDARY),
            "handover": lambda w: ma.raise_if(w),                   # (and remesh: both decode with the defaults)
            "tracking": lambda w: ma.raise_if(w, **tracking._ERR),
            "evaluate": lambda w: ma.raise_if(w, **evaluate._ERR),
            "density": lambda w: ma.raise_if(w, **density.ERR_TEXTS)}


@pytest.mark.parametrize("user", sorted(TABLE))
def test_decoder_reproduces_every_users_table(user):
    decode = _decoders()[user]
    assert len(TABLE[user]) == 16
    for word, want in enumerate(TABLE[user]):
        if want is OK:
            decode(word)
        else:
            with pytest.raises(ValueError) as ex:
                decode(word)
            assert str(ex.value) == want, (user, word)


def test_constants_are_the_headers():
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "gaustar_amd", "csrc", "gsr_mesh.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (MESH_ERR_\w+) = (\d+);", src)}
    assert header == {"MESH_ERR_INDEX": 1, "MESH_ERR_NAN": 2, "MESH_ERR_DUP": 4, "MESH_ERR_DEGENERATE": 8}
    assert all(getattr(ma, name) == value for name, value in header.items())


def test_meshargs_imports_no_feature_module():
    import os
    src = open(os.path.join(os.path.dirname(ma.__file__), "_meshargs.py")).read()
    assert "from ." not in src and "import gaustar_amd" not in src


def _raises(kind, text, fn, *args):
    with pytest.raises(kind) as ex:
        fn(*args)
    assert type(ex.value) is kind and str(ex.value) == text


def test_faces_i32():
    _raises(ValueError, "faces must be [F,3]", ma.faces_i32, torch.zeros(4, 2, dtype=torch.int32))
    _raises(ValueError, "faces must be [F,3]", ma.faces_i32, torch.zeros(6, dtype=torch.int32))
    _raises(ValueError, "faces must be int32 or int64", ma.faces_i32, torch.zeros(4, 3, dtype=torch.float32))
    _raises(RuntimeError, "the mesh must be on a GPU", ma.faces_i32, torch.zeros(4, 3, dtype=torch.int32))
    _raises(RuntimeError, "the mesh must be on a GPU", ma.faces_i32, torch.zeros(4, 3, dtype=torch.int64))
    many = torch.zeros(1, 3, dtype=torch.int32).expand(ma.MAX_FACES + 1, 3)
    _raises(ValueError, f"{ma.MAX_FACES + 1} faces: more than 2^31 / 3, the face-edges cannot be indexed in int32", ma.faces_i32, many)
    assert ma.MAX_FACES == (2 ** 31 - 1) // 3


def test_verts_f32():
    cpu, gpu = torch.device("cpu"), torch.device("cuda", 0)
    _raises(ValueError, "verts must be [V,3] float32", ma.verts_f32, torch.zeros(5, 3, dtype=torch.float64), cpu)
    _raises(ValueError, "verts must be [V,3] float32", ma.verts_f32, torch.zeros(5, 2), cpu)
    _raises(RuntimeError, "verts and faces must be on the same GPU", ma.verts_f32, torch.zeros(5, 3), gpu)
    v = torch.zeros(5, 6)[:, ::2].requires_grad_()
    out = ma.verts_f32(v, cpu)
    assert out.is_contiguous() and not out.requires_grad and out.shape == (5, 3)


def test_mask_u8():
    cpu, gpu = torch.device("cpu"), torch.device("cuda", 0)
    assert ma.mask_u8(None, 4, cpu) is None
    _raises(ValueError, "mask must be [F] bool or uint8", ma.mask_u8, torch.zeros(5, dtype=torch.bool), 4, cpu)
    _raises(ValueError, "mask must be [F] bool or uint8", ma.mask_u8, torch.zeros(4, dtype=torch.int32), 4, cpu)
    _raises(RuntimeError, "mask and faces must be on the same GPU", ma.mask_u8, torch.zeros(4, dtype=torch.bool), 4, gpu)
    m = torch.tensor([True, False, True, True])
    out = ma.mask_u8(m, 4, cpu)
    assert out.dtype == torch.uint8 and out.tolist() == [1, 0, 1, 1] and out.data_ptr() == m.data_ptr()
    u = torch.tensor([1, 0, 2, 0], dtype=torch.uint8)
    assert ma.mask_u8(u, 4, cpu).data_ptr() == u.data_ptr()


def test_mesh_f64_and_points_f64():
    on_gpu = "verts and faces must be tensors on a GPU"
    _raises(ValueError, on_gpu, ma.mesh_f64, torch.zeros(5, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.int32))
    _raises(ValueError, on_gpu, ma.mesh_f64, [[0.0, 0.0, 0.0]], torch.zeros(4, 3, dtype=torch.int32))
    _raises(ValueError, on_gpu, ma.mesh_f64, torch.zeros(5, 3, dtype=torch.float64), [[0, 1, 2]])
    cpu = torch.device("cpu")
    _raises(ValueError, "pos must be [K,3] float64 on the tracker's GPU", ma.points_f64, torch.zeros(5, 3), cpu, "pos")
    _raises(ValueError, "points must be [K,3] float64 on the tracker's GPU", ma.points_f64, torch.zeros(5, 2, dtype=torch.float64), cpu,
            "points")
    _raises(ValueError, "points must be [K,3] float64 on the tracker's GPU", ma.points_f64, torch.zeros(5, 3, dtype=torch.float64),
            torch.device("cuda", 0), "points")
    assert ma.points_f64(torch.zeros(5, 3, dtype=torch.float64), cpu, "pos").shape == (5, 3)


def test_new_err():
    err = ma.new_err("cpu")
    assert err.dtype == torch.int32 and err.tolist() == [0]
