"""A float64 torch restatement of the regularisers on the Gaussians' own parameters (gaustar_trainers/refine.py:739-740,
:743-748, :663-669), gradients by autograd.  Shared by tests/test_param_reg_host.py (CPU) and tests/test_gpu_param_reg.py."""
import torch


def ref_parts(delta_t=None, delta_r=None, weight=None, factor_t=100.0, factor_r=1.0, densities=None, min_opacity=0.8,
              sh_dc=None, pre_sh_dc=None, sh_factor=1.0):
    """-> [loose_t, loose_r, opacity, sh] as 0-dim f64 tensors (0 for a term that is left out).  delta_t [N,3], delta_r [N,4],
    weight [N] or [N,3] or None, densities [N] or [N,1], sh_dc [N,3] or [N,1,3], pre_sh_dc [M,3] or [M,1,3]."""
    some = next(t for t in (delta_t, delta_r, densities, sh_dc) if t is not None)
    zero = torch.zeros((), dtype=torch.float64, device=some.device)
    d = lambda t: t.double()
    w = None
    if weight is not None:
        w = d(weight)
        w = w[:, None].expand(-1, 3) if w.dim() == 1 else w.expand(-1, 3)
    one = torch.ones((), dtype=torch.float64, device=some.device)
    parts = [zero, zero, zero, zero]
    if delta_t is not None and factor_t != 0.0:
        parts[0] = factor_t * ((one if w is None else w) * d(delta_t).abs()).mean()                      # :739
    if delta_r is not None and factor_r != 0.0:
        parts[1] = factor_r * ((one if w is None else w) * d(delta_r)[..., 1:].abs()).mean()             # :740
    if densities is not None:
        strengths = torch.sigmoid(d(densities)).view(-1, 1)
        parts[2] = torch.relu(min_opacity - strengths).mean()                                          # :748
    if sh_dc is not None and pre_sh_dc is not None and sh_factor != 0.0 and pre_sh_dc.numel():
        pre = d(pre_sh_dc).reshape(-1, 3)
        parts[3] = sh_factor * ((pre - d(sh_dc).reshape(-1, 3)[:pre.shape[0]]) ** 2).mean()             # :667 / :669
    return parts


def ref_total(**kw):
    p = ref_parts(**kw)
    return ((p[0] + p[1]) + p[2]) + p[3]
