"""RAFT optical flow without a GPU: tests/flow_ref.py in f64 against the fixture the reference's own RAFT wrote
(tests/golden/make_flow_golden.py), the checkpoint loader's checks, the pad split and the box mean's rounding."""
import os

import numpy as np
import pytest
import torch

import flow_ref
from conftest import GOLDEN_DIR

KAT = os.path.join(GOLDEN_DIR, "flow", "flow_kat.npz")
STAGES = (1, 4, 20)


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(KAT))


@pytest.mark.parametrize("case", ["A", "B"])
def test_restatement_in_f64_matches_the_reference(kat, case):
    """Per stage k: D_k = max|fixture - ref64| <= 4 s_k, s_k the reference's own sensitivity to a relative 2^-23 in every
    weight.  The reference's f32-to-f64 distance is 1.3 - 1.8 s_k (measured: 2.3e-6 / 4.4e-6 / 1.7e-5 px in case A); a wrong
    window order or pad split is off by whole pixels."""
    assert tuple(kat["stages"]) == STAGES
    sd = flow_ref.seeded_state_dict(float(kat[f"{case}_gain"]))
    out = flow_ref.raft(sd, kat[f"{case}_image1"], kat[f"{case}_image2"], iters=20, stages=STAGES, dtype=torch.float64)
    for k in STAGES:
        want = kat[f"{case}_flow_{k}"]
        assert out[k].shape == want.shape == (125, 134, 2)
        D = float(np.abs(out[k].numpy() - want.astype(np.float64)).max())
        s = float(kat[f"{case}_s_{k}"])
        print(f"case {case} k={k}: D_k = {D:.3e}  s_k = {s:.3e}  max|flow| = {np.abs(want).max():.2f}")
        assert D <= 4.0 * s, (case, k, D, s)


def test_fixture_conditions(kat):
    assert kat["A_s_20"] <= 1e-4 and 2.0 <= np.abs(kat["A_flow_20"]).max() <= 32.0
    assert kat["B_s_20"] <= 1e-3 and np.abs(kat["B_flow_20"]).max() >= 64.0
    assert os.path.getsize(KAT) < 1_000_000


def test_pad_split_for_every_residue():
    """InputPadder, 'sintel': pad//2 before, the rest after."""
    from gaustar_amd.flow import pad_split
    want = {0: (0, 0), 1: (3, 4), 2: (3, 3), 3: (2, 3), 4: (2, 2), 5: (1, 2), 6: (1, 1), 7: (0, 1)}
    for r, (before, after) in want.items():
        for n in (128 + r, 536 + r):
            assert pad_split(n) == (before, after), n
            assert (n + before + after) % 8 == 0
    img = np.arange(125 * 134 * 3, dtype=np.int64).reshape(125, 134, 3).astype(np.uint8)
    x = flow_ref.prep_image(img, 1)
    assert tuple(x.shape) == (128, 136, 3)
    assert torch.equal(x[0], x[1]) and torch.equal(x[-1], x[-3]) and torch.equal(x[:, 0], x[:, 1]) and torch.equal(x[:, -1], x[:, -2])
    assert torch.equal(x[1:126, 1:135], 2.0 * (torch.from_numpy(img).double() / 255.0) - 1.0)


def test_box_mean_rounds_half_to_even():
    img = np.zeros((2, 8, 3), np.uint8)
    # 2 x 2 sums 2, 6, 10, 14: means 0.5, 1.5, 2.5, 3.5 -> 0, 2, 2, 4
    for j, s in enumerate((2, 6, 10, 14)):
        img[0, 2 * j, :] = s
    assert flow_ref.box_mean(img, 2)[0, :, 0].tolist() == [0, 2, 2, 4]
    img[0, 0, :] = 3                                       # 0.75 -> 1
    img[0, 2, :] = 5                                       # 1.25 -> 1
    assert flow_ref.box_mean(img, 2)[0, :2, 1].tolist() == [1, 1]
    big = np.zeros((4, 4, 3), np.uint8)
    big[0, 0] = 8                                          # 8 / 16 = 0.5 -> 0
    assert flow_ref.box_mean(big, 4)[0, 0].tolist() == [0, 0, 0]
    big[0, 1] = 16                                         # 24 / 16 = 1.5 -> 2
    assert flow_ref.box_mean(big, 4)[0, 0].tolist() == [2, 2, 2]
    rng = np.random.default_rng(0)
    r = rng.integers(0, 256, (6, 10, 3), dtype=np.uint8)
    assert np.array_equal(flow_ref.box_mean(r, 1), r)
    exact = r.astype(np.float64).reshape(3, 2, 5, 2, 3).mean((1, 3))
    assert np.array_equal(flow_ref.box_mean(r, 2), np.round(exact).astype(np.uint8))      # numpy rounds half to even too


def test_loader_checks_every_key_and_shape():
    from gaustar_amd import flow
    sd = flow_ref.seeded_state_dict(1.0)
    assert set(flow.check_state_dict(sd)) == set(flow.expected_shapes())
    pre = {"module." + k: v for k, v in sd.items()}
    pre["module.cnet.norm1.num_batches_tracked"] = torch.tensor(0)
    got = flow.check_state_dict(pre)
    assert set(got) == set(sd) and all(got[k] is sd[k] for k in sd)
    missing = dict(sd)
    del missing["update_block.gru.convq2.bias"]
    with pytest.raises(ValueError, match="update_block.gru.convq2.bias.*missing"):
        flow.check_state_dict(missing)
    wrong = dict(sd)
    wrong["fnet.layer2.0.conv1.weight"] = torch.zeros(96, 64, 3, 1)
    with pytest.raises(ValueError, match=r"fnet.layer2.0.conv1.weight.*\(96, 64, 3, 3\).*\(96, 64, 3, 1\)"):
        flow.check_state_dict(wrong)
    extra = dict(sd)
    extra["update_block.extra.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="unexpected key 'update_block.extra.weight'"):
        flow.check_state_dict(extra)
    ints = dict(sd)
    ints["fnet.conv1.bias"] = torch.zeros(64, dtype=torch.int32)
    with pytest.raises(ValueError, match="floating point"):
        flow.check_state_dict(ints)
    with pytest.raises(ValueError, match="state dict"):
        flow.check_state_dict([1, 2])


def test_small_model_is_refused_as_such():
    from gaustar_amd import flow
    small = {"module.fnet.conv1.weight": torch.zeros(32, 3, 7, 7), "module.update_block.gru.convz.weight": torch.zeros(96, 242, 3, 3)}
    with pytest.raises(ValueError, match="--small"):
        flow.check_state_dict(small)
    with pytest.raises(ValueError, match="--small"):
        flow.check_state_dict({"fnet.conv1.weight": torch.zeros(32, 3, 7, 7)})


def test_lookup_window_order_is_the_references():
    """Channel 9 i + j of a level samples at (x + d_i, y + d_j): on a map that grows along x only, the FIRST index moves the value."""
    level = torch.arange(12, dtype=torch.float64)[None, None, :].expand(1, 10, 12).contiguous()     # value = x
    levels = [level, level[:, :5, :6], level[:, :2, :3], level[:, :1, :1]]
    out = flow_ref.lookup(levels, torch.tensor([[5.0, 4.0]], dtype=torch.float64))[0, :81].reshape(9, 9)
    assert torch.equal(out[:, 0], torch.arange(1, 10, dtype=torch.float64)) and torch.equal(out[:, 3], out[:, 0])


def test_entry_points_validate_without_gpu(hip_lib):
    """Argument checks come before any device work."""
    import ctypes
    from gaustar_amd._lib import FlowConvDesc, FlowSlice
    err = hip_lib.gsr_last_error
    assert hip_lib.gsr_flow_packed_k(147) == 160 and hip_lib.gsr_flow_packed_k(324) == 336 and hip_lib.gsr_flow_packed_n(2) == 4 and hip_lib.gsr_flow_packed_n(5) == 64
    assert hip_lib.gsr_flow_packed_n(576) == 576 and hip_lib.gsr_flow_packed_n(126) == 128
    assert hip_lib.gsr_flow_conv(None, None) != 0 and b"null" in err()
    d = FlowConvDesc()
    assert hip_lib.gsr_flow_conv(ctypes.addressof(d), None) != 0 and b"positive" in err()
    d.N = d.H = d.W = 1
    d.KH, d.KW, d.stride = 3, 1, 1
    assert hip_lib.gsr_flow_conv(ctypes.addressof(d), None) != 0 and b"1x1, 3x3, 7x7, 1x5 or 5x1" in err()
    d.KW, d.stride = 3, 3
    assert hip_lib.gsr_flow_conv(ctypes.addressof(d), None) != 0 and b"stride must be 1 or 2" in err()
    d.stride, d.n_in, d.Cout = 1, 1, 1
    assert hip_lib.gsr_flow_conv(ctypes.addressof(d), None) != 0 and b"Cout must be between 2 and 576" in err()
    d.Cout = 8
    assert hip_lib.gsr_flow_conv(ctypes.addressof(d), None) != 0 and b"null" in err()
    assert hip_lib.gsr_flow_prep_image(8, 8, None, 3, None, None) != 0 and b"factor must be 1, 2 or 4" in err()
    assert hip_lib.gsr_flow_prep_image(9, 8, None, 2, None, None) != 0 and b"multiple of factor" in err()
    assert hip_lib.gsr_flow_prep_image(8, 8, None, 2, None, None) != 0 and b"null" in err()
    assert hip_lib.gsr_flow_corr_volume(4, 4, 128, None, None, None, None) != 0 and b"null" in err()
    assert hip_lib.gsr_flow_corr_pool(4, 1, 8, None, None, None) != 0 and b"at least 2 x 2" in err()
    assert hip_lib.gsr_flow_instance_norm(1, 4, 6, None, 0, None, None, None, None) != 0 and b"multiple of 4" in err()
    assert hip_lib.gsr_flow_instance_norm_workspace_bytes(2, 300, 96) >= 2 * 96 * 2 * 32 + 2 * 96 * 8
    assert hip_lib.gsr_flow_gru_combine(4, 2, None, None, None, None, None) != 0 and b"mode" in err()
    s = FlowSlice(None, 4, 0, 3)
    assert hip_lib.gsr_flow_upsample(2, 2, ctypes.addressof(s), None, 0, 0, 17, 16, None, None) != 0 and b"inside the padded" in err()
    assert hip_lib.gsr_flow_upsample(2, 2, ctypes.addressof(s), None, 0, 0, 16, 16, None, None) != 0 and b"null" in err()
    assert hip_lib.gsr_flow_corr_lookup(2, 2, 4, 8, None, None, None, None, None, None, None) != 0 and b"levels" in err()


def test_seeded_weights_are_reproducible():
    a, b = flow_ref.seeded_state_dict(0.6), flow_ref.seeded_state_dict(0.6)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(a["cnet.layer2.0.norm3.weight"], a["cnet.layer2.0.downsample.1.weight"])
    assert (a["cnet.norm1.running_var"] >= 0.5).all() and (a["cnet.norm1.running_var"] <= 1.5).all()
    w = a["update_block.encoder.convc2.weight"]
    assert abs(float(w.std()) * np.sqrt(256 * 9) / 0.6 - 1.0) < 0.02
