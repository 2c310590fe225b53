"""The inverse-CDF fine sampler (`fine_sampler = "pdf"`) without a GPU: its torch restatement (tests/pdf_ref.py) on cases that can
be checked by hand, the two sys_param keys at model construction, the op's refusal of CPU tensors and the sampler kernel's
register budget in the compiled gfx950 object."""
import os

import pytest
import torch

from mc_nerf_amd import synthetic as S
from pdf_ref import sample_pdf_ref, split_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(Sc, near=2.0, far=6.0):
    return torch.linspace(near, far, Sc)


def test_uniform_weights_spread_samples_evenly_over_the_interior_bins():
    Sc, I = 10, 80                      # 8 interior bins between the 9 edges mid[0] .. mid[8]
    z = _grid(Sc)
    w = torch.full((1, Sc), 0.3)
    u = (torch.arange(I, dtype=torch.float32) + 0.5).unsqueeze(0) / I
    z_all, zs, zc = sample_pdf_ref(w, z, None, u)
    mid = 0.5 * (z[:-1] + z[1:])
    assert torch.equal(zc[0], z)
    counts = torch.histc(zs[0], bins=Sc - 2, min=float(mid[0]), max=float(mid[-1]))
    assert torch.equal(counts, torch.full((Sc - 2,), I / (Sc - 2)))
    # equal weights: the inverse CDF is linear, u -> mid[0] + u (mid[-1] - mid[0])
    assert torch.allclose(zs[0], mid[0] + u[0] * (mid[-1] - mid[0]), atol=2e-6)
    assert torch.equal(z_all, torch.sort(torch.cat([zc, zs], 1), 1).values)


def test_one_spike_puts_every_sample_inside_its_bin():
    Sc, I = 16, 200
    z = _grid(Sc)
    w = torch.zeros(1, Sc)
    w[0, 7] = 1.0                       # wb[6]: the bin between mid[6] and mid[7]
    u = torch.rand(1, I, generator=torch.Generator().manual_seed(0))
    _, zs, _ = sample_pdf_ref(w, z, None, u)
    mid = 0.5 * (z[:-1] + z[1:])
    pdf_spike = (1.0 + 1e-5) / (1.0 + 1e-5 * (Sc - 2))
    inside = (zs >= mid[6]) & (zs <= mid[7])
    # the floored bins hold 1e-5 each: a u below cdf[6] or above cdf[7] lands in them (their pdf < 1e-5: denom 1, t tiny)
    lo, hi = 6 * 1e-5 / (1.0 + 1e-5 * (Sc - 2)), 6 * 1e-5 / (1.0 + 1e-5 * (Sc - 2)) + pdf_spike
    assert bool(inside[(u >= lo) & (u < hi)].all()) and int(inside.sum()) >= I - 1


def test_all_zero_weights_fall_back_to_the_floor():
    Sc, I = 12, 50
    z = _grid(Sc)
    u = torch.rand(3, I, generator=torch.Generator().manual_seed(1))
    a = sample_pdf_ref(torch.zeros(3, Sc), z, None, u)[1]
    b = sample_pdf_ref(torch.full((3, Sc), 7.0), z, None, u)[1]             # any constant weight: the same uniform pdf
    mid = 0.5 * (z[:-1] + z[1:])
    assert torch.isfinite(a).all() and torch.allclose(a, b, atol=1e-6)
    assert torch.allclose(a, mid[0] + u * (mid[-1] - mid[0]), atol=2e-6)


def test_u_one_yields_the_last_edge_and_u_zero_the_first():
    Sc = 9
    z = _grid(Sc)
    jit = torch.tensor([0.0, 0.1, 0.37])
    w = torch.rand(3, Sc, generator=torch.Generator().manual_seed(2))
    u = torch.tensor([[1.0, 0.0]] * 3)
    z_all, zs, zc = sample_pdf_ref(w, z, jit, u)
    mid = 0.5 * (zc[:, :-1] + zc[:, 1:])
    assert torch.allclose(zs[:, 0], mid[:, -1], atol=1e-6, rtol=0) and torch.equal(zs[:, 1], mid[:, 0])
    assert torch.equal(zc, z.unsqueeze(0) + jit.unsqueeze(1))
    assert z_all.shape == (3, Sc + 2) and bool((z_all[:, 1:] >= z_all[:, :-1]).all())
    zs_sorted, zc_found = split_rows(z_all, zc)
    assert torch.equal(zc_found, zc) and torch.equal(zs_sorted, torch.sort(zs, 1).values)


def _nerf(**kw):
    from mc_nerf_amd.model import NeRF_Model
    sp = S.make_sys_param("cpu", samples=kw.pop("samples", 32), scale=2, batch=16, H=8, W=8, coarse=(4, 32, [2]), fine=(8, 64, [4]))
    sp.update(kw)
    return NeRF_Model(sp)


def test_fine_sampler_keys_reach_the_settings():
    m = _nerf()
    assert m.settings.fine_sampler == "threshold" and m.fine_sampler == "threshold" and m.settings.n_importance == 128
    m = _nerf(fine_sampler="pdf", n_importance=96)
    assert (m.settings.fine_sampler, m.settings.n_importance, m.settings.samples_pdf) == ("pdf", 96, 32 + 96)
    assert m.settings.pdf and m.last_selection is None
    m = _nerf(fine_sampler="threshold", n_importance=5)
    assert not m.settings.pdf and m.settings.samples_f == 64
    m = _nerf(samples=2, fine_sampler="threshold")          # the threshold sampler keeps taking any coarse count
    assert m.settings.samples_c == 2


@pytest.mark.parametrize("kw, key", [(dict(fine_sampler="importance"), "fine_sampler"), (dict(fine_sampler=None), "fine_sampler"),
                                     (dict(fine_sampler="pdf", n_importance=0), "n_importance"),
                                     (dict(n_importance=-3), "n_importance"), (dict(fine_sampler="pdf", n_importance=2.5), "n_importance"),
                                     (dict(fine_sampler="pdf", samples=2), "samples"),
                                     (dict(fine_sampler="pdf", samples=64, n_importance=961), "n_importance")])
def test_bad_fine_sampler_settings_are_refused(kw, key):
    with pytest.raises(ValueError, match=key):
        _nerf(**kw)


def test_the_bound_itself_is_accepted():
    from mc_nerf_amd import ops
    m = _nerf(fine_sampler="pdf", samples=64, n_importance=ops.PDF_MAX_SAMPLES - 64)
    assert m.settings.samples_pdf == ops.PDF_MAX_SAMPLES == 1024


def test_sample_pdf_refuses_cpu_tensors():
    from mc_nerf_amd import _lib, ops
    with pytest.raises(_lib.McnerfError):
        ops.sample_pdf(torch.rand(4, 16), _grid(16), None, torch.rand(4, 8))
    with pytest.raises(_lib.McnerfError):
        ops.sample_pdf(torch.rand(4, 16), _grid(16), torch.zeros(4), torch.rand(4, 8))


def test_sampler_kernel_uses_no_scratch(tmp_path):
    """Same method as tests/test_build_invariants_cpu.py: the gfx950 code object's kernel descriptors."""
    from test_build_invariants_cpu import _device_elf, _kernel_meta
    meta = _kernel_meta(_device_elf("sample_pdf.o", str(tmp_path)))
    assert list(meta) == ["_Z17sample_pdf_kernel16McnSamplePdfArgs"]
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_abi_declares_the_sampler():
    from mc_nerf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcnerf.h")).read()
    assert "int mcnerf_sample_pdf(" in hdr and hasattr(_lib.lib(), "mcnerf_sample_pdf")
    assert _lib.ABI_VERSION == 7                             # (new symbols only; tests/test_abi_cpu.py checks header, table and library)
