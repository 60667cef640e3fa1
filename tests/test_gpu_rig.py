"""GPU: the one device rule (gaustar_amd._host.resolve_device) and the one sweep over a shard's cameras
(gaustar_amd.sweep.run_cameras).  What the rig passes compute through them is pinned bit for bit by their own suites."""
import numpy as np
import pytest
import torch

from gaustar_amd import _host, sweep

pytestmark = pytest.mark.gpu


def test_resolve_device_is_indexed_and_equals_a_tensors_device():
    t = torch.zeros(1, device="cuda")
    for dev in (_host.resolve_device(None, what="X"), _host.resolve_device("cuda", what="X"), _host.resolve_device(like=t, what="X"),
                _host.resolve_device(None, np.zeros(1), what="X"), _host.resolve_device(None, torch.zeros(1), what="X", exc=ValueError)):
        assert dev.index is not None and dev == t.device
    last = torch.device("cuda", torch.cuda.device_count() - 1)
    assert _host.resolve_device(last, t, what="X") == last                  # an explicit device wins over the tensor's


@pytest.mark.parametrize("views_in_flight", [1, 2])
def test_run_cameras_visits_every_camera_of_the_shard_once(views_in_flight):
    dev = torch.device("cuda", torch.cuda.current_device())
    images = torch.arange(5 * 6 * 8, dtype=torch.float32, device=dev).view(5, 6, 8)
    shard = [4, 0, 2]                                                       # 3 cameras of 6 x 8, not in order
    sums = torch.zeros(len(shard), device=dev)
    seen = []

    def per_camera(j, i):
        assert torch.cuda.current_device() == dev.index
        seen.append((j, i))                                                 # (list.append is atomic; the order is the workers')
        sums[j] = images[i].sum()

    sweep.run_cameras(shard, per_camera, views_in_flight, dev)
    torch.cuda.synchronize(dev)
    assert sorted(seen) == [(0, 4), (1, 0), (2, 2)]
    assert torch.equal(sums.cpu(), images[shard].sum((1, 2)).cpu())
    assert torch.cuda.current_device() == dev.index
    sweep.run_cameras([], per_camera, views_in_flight, dev)
    assert len(seen) == 3


def test_run_cameras_restores_the_current_device():
    if torch.cuda.device_count() < 2:
        other = torch.device("cuda", torch.cuda.current_device())
    else:
        other = torch.device("cuda", (torch.cuda.current_device() + 1) % torch.cuda.device_count())
    before = torch.cuda.current_device()
    inside = []
    sweep.run_cameras([0, 1, 2], lambda j, i: inside.append(torch.cuda.current_device()), 1, other)
    assert inside == [other.index] * 3 and torch.cuda.current_device() == before
