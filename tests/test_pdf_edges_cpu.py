"""The inputs of tests/test_pdf_edges_gpu.py without a GPU (tests/pdf_edge_cases.py): the caps of `check_rows` (every sample inside
the u +- 1e-6 bracket, 99.9 % within 2e-6) are conditions, so the arithmetic choices the sampler's contract leaves open must not be
able to use them up.  Every case of the table is evaluated a second time on the CPU with exactly those choices made differently --
the total and the CDF summed in 64-element chunks with an fp64 carry and another order inside a chunk, the last line in fp64 -- and
must agree with the restatement (tests/pdf_ref.py) far inside the caps.  Also: the `out=` argument of ops.sample_pdf refuses a wrong
buffer before the library is called, and `pdf_cdf_ref` gives the numbers of a case that can be worked out by hand."""
import pytest
import torch

import pdf_edge_cases as C
from pdf_ref import pdf_cdf_ref, sample_pdf_ref
from test_pdf_sampler_gpu import check_rows


def _scan64(x):
    """Inclusive sum of x [n, m <= 64] (fp64) by doubling steps: the association of a wavefront scan, not cumsum's left to right."""
    d = 1
    while d < x.shape[1]:
        x = x + torch.cat([torch.zeros_like(x[:, :d]), x[:, :-d]], 1)
        d *= 2
    return x


def pdf_cdf_chunked(w):
    """pdf_cdf_ref's contract with the sums taken as the kernel may take them: chunks of 64 with an fp64 carry, the total of a chunk
    from its last element backwards, the running sum of a chunk by doubling steps."""
    wb = w.float()[:, 1:-1] + 1e-5
    n, nb = wb.shape
    tot = torch.zeros(n, dtype=torch.float64)
    for b in range(0, nb, 64):
        tot = tot + wb[:, b:b + 64].double().flip(-1).cumsum(-1)[:, -1]
    pdf = wb / tot.float().unsqueeze(1)
    cdf = torch.zeros(n, nb + 1)
    carry = torch.zeros(n, 1, dtype=torch.float64)
    for b in range(0, nb, 64):
        inc = _scan64(pdf[:, b:b + 64].double())
        cdf[:, b + 1:b + 1 + inc.shape[1]] = (carry + inc).float()
        carry = carry + inc[:, -1:]
    return pdf, cdf


def sample_pdf_alt(w, zgrid, jitter, u):
    """The contract of sample_pdf_ref on pdf_cdf_chunked's sums, the last line as float(double(m_lo) + double(t) * double(m_hi - m_lo))
    -> (z_all sorted, cdf)."""
    n, Sc = w.shape
    u = u.float()
    mid = C.edges_ref(zgrid, jitter, n)
    zc = zgrid.reshape(1, Sc).float() + (torch.zeros(n) if jitter is None else jitter.reshape(n).float()).unsqueeze(1)
    pdf, cdf = pdf_cdf_chunked(w)
    ind = torch.searchsorted(cdf, u.contiguous(), right=True)
    below, above = (ind - 1).clamp(min=0), ind.clamp(max=Sc - 2)
    interior = (ind >= 1) & (ind <= Sc - 2)
    denom = torch.where(interior, pdf.gather(1, (ind - 1).clamp(0, Sc - 3)), torch.zeros_like(u))
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf.gather(1, below)) / denom
    m_lo, m_hi = mid.gather(1, below), mid.gather(1, above)
    zs = (m_lo.double() + t.double() * (m_hi - m_lo).double()).float()
    return torch.sort(torch.cat([zc, zs], -1), -1).values, cdf


@pytest.mark.parametrize("Sc, I", C.SHAPES)
def test_the_table_leaves_the_caps_unused(Sc, I):
    """Per case: the CDF entries bit-equal, 100 % of the samples within 2e-6, none outside the bracket, the coarse depths found bit
    for bit (check_rows asserts the last two and sortedness, and returns the share)."""
    names = []
    for name, w, zgrid, jit, u in C.cases(Sc, I):
        z_alt, cdf = sample_pdf_alt(w, zgrid, jit, u)
        assert C.same_bits(cdf, pdf_cdf_ref(w)[1]), name
        assert check_rows(z_alt, w, zgrid, jit, u) == 1.0, name
        names.append(name)
    assert len(names) == len(C.WEIGHTS) * (len(C.DRAWS) + 1)


def test_the_table_holds_what_it_says():
    assert len(C.SHAPES) == 19 and len(set(C.SHAPES)) == 19 and all(3 <= Sc and 1 <= I and Sc + I <= 1024 for Sc, I in C.SHAPES)
    assert all(Sc + I == 1024 for Sc, I in C.GROUPS["bound"]) and C.N % 4 == 1
    lds = lambda Sc, I: 4 * (4 * ((Sc + 3) & ~3) + ((I + 3) & ~3)) * 4
    assert all(lds(*s) == 65600 for s in C.BIG_LDS) and lds(*C.UNDER_BIG_LDS) == 65344
    assert [s for s in C.SHAPES if lds(*s) > 65536] == C.BIG_LDS
    Sc, I = 130, 33
    gen = C.gen_of(Sc, I)
    w = C.weights_of("onehot", Sc, gen)
    assert int(w[0].argmax()) == 0 and int(w[1].argmax()) == Sc - 1 and bool((w.sum(1) == 1).all())
    # a spike outside the interior: the uniform floor
    assert C.same_bits(pdf_cdf_ref(w[:2])[0], pdf_cdf_ref(torch.zeros(2, Sc))[0])
    peaky = pdf_cdf_ref(C.weights_of("peaky", Sc, gen))[0]
    assert float((peaky < 1e-5).float().mean()) > 0.5
    w = C.weights_of("random", Sc, gen)
    cdf = pdf_cdf_ref(w)[1]
    u = C.draws_of("on_cdf", w, I, gen)
    on = (u.unsqueeze(2) == cdf.unsqueeze(1)).any(2)
    assert 0.3 < float(on.float().mean()) < 0.4 and bool(on[0, 0::3].all()) and not bool(on[0, 1::3].any() or on[0, 2::3].any())
    assert bool((u[0, 1::3] > u[0, 0::3][:u[0, 1::3].numel()]).all()) and bool((u[0, 2::3] < u[0, 0::3][:u[0, 2::3].numel()]).all())
    u = C.draws_of("ties", w, I, gen)
    assert all(bool((u[r] == u[r, 0]).all()) for r in C.TIES_EQUAL_ROWS)
    dup = torch.tensor([I - u[r].unique().numel() for r in range(1, C.N - 1)])
    assert bool((dup == 3).all())                                          # a pair and a triple
    assert not bool((u[1:-1, 1:] >= u[1:-1, :-1]).all(1).any())            # unsorted
    u = C.draws_of("outside", w, I, gen)
    for v in C.OUTSIDE:
        hit = (u == v) & (torch.signbit(u) == (v < 0 or str(v) == "-0.0"))
        assert 0.05 < float(hit.float().mean()) < 0.12
    assert torch.equal(C.draws_of("linspace", w, I, gen)[5], torch.linspace(0, 1, I))


def test_pdf_cdf_ref_on_one_spike_by_hand():
    """The numbers of test_pdf_sampler_cpu.py::test_one_spike_puts_every_sample_inside_its_bin: Sc = 16, a spike of 1 at index 7
    (interior bin 6), 14 interior bins floored at 1e-5."""
    Sc = 16
    w = torch.zeros(1, Sc)
    w[0, 7] = 1.0
    pdf, cdf = pdf_cdf_ref(w)
    assert pdf.shape == (1, Sc - 2) and cdf.shape == (1, Sc - 1)
    tot = 1.0 + 1e-5 * (Sc - 2)
    want = torch.full((Sc - 2,), 1e-5 / tot, dtype=torch.float64)
    want[6] = (1.0 + 1e-5) / tot
    assert torch.allclose(pdf[0].double(), want, rtol=3e-7, atol=0)
    assert float(cdf[0, 0]) == 0.0 and torch.allclose(cdf[0, 1:].double(), want.cumsum(0), rtol=3e-7, atol=1e-12)
    assert abs(float(cdf[0, 6]) - 6e-5 / tot) < 1e-11 and abs(float(cdf[0, 7]) - (6e-5 + 1.0 + 1e-5) / tot) < 3e-7
    assert abs(float(cdf[0, -1]) - 1.0) < 3e-7              # (fp32: 1 + 1e-5 and the quotient are each rounded at 6e-8)
    # sample_pdf_ref is built on it
    u = torch.tensor([[0.5]])
    zs = sample_pdf_ref(w, C.zgrid_of(Sc), None, u)[1]
    mid = C.edges_ref(C.zgrid_of(Sc), None, 1)
    t = (0.5 - float(cdf[0, 6])) / float(pdf[0, 6])
    assert abs(float(zs) - (float(mid[0, 6]) + t * float(mid[0, 7] - mid[0, 6]))) < 1e-6


@pytest.mark.parametrize("bad", ["shape", "rows", "dtype", "device", "strided"])
def test_out_refuses_a_wrong_buffer_before_the_library_is_called(bad, monkeypatch):
    from mc_nerf_amd import _lib, ops
    N, Sc, I = 4, 16, 8
    out = {"shape": lambda: torch.empty(N, Sc + I + 1), "rows": lambda: torch.empty(N + 1, Sc + I),
           "dtype": lambda: torch.empty(N, Sc + I, dtype=torch.float64), "device": lambda: torch.empty(N, Sc + I, device="meta"),
           "strided": lambda: torch.empty(N, 2 * (Sc + I))[:, ::2]}[bad]()
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("the library was called"))
    with pytest.raises(_lib.McnerfError, match="out must be"):
        ops.sample_pdf(torch.rand(N, Sc), C.zgrid_of(Sc), None, torch.rand(N, I), out=out)
