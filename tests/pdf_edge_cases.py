"""Shapes, weights and draws shared by tests/test_pdf_edges_cpu.py and tests/test_pdf_edges_gpu.py (the inverse-CDF sampler,
mc_nerf_amd/csrc/sample_pdf.hip, beyond one 64-lane chunk and at its edges).  Plain data and builders on the CPU: no GPU, no fixtures.

The kernel runs one wavefront per ray and walks the ray in chunks of 64 lanes, carrying the fp64 total of the floored weights, the
CDF and the merge's histogram prefix from chunk to chunk; four rays share a workgroup.  The shapes (Sc, I):
  * tiny: one interior bin (Sc = 3), I < 64, I and Sc no multiple of 4 (the padding of the LDS regions);
  * around one chunk: Sc = 65 is the first second chunk of the depth loop and of the merge's scan, Sc = 67 (Sc - 2 = 65 interior
    bins) the first use of the CDF carry;
  * several chunks, ragged and full, in Sc and in I;
  * the bound Sc + I = 1024; Sc >= 1021 takes more than 64 KiB of LDS (4 waves x (4 * 1024 + 4) floats), (1020, 4) sits just under.
N = 257 rays: the last workgroup holds one ray and three idle waves.

Weights: `random`; `zero`; `onehot` (a random position, ends included: a spike at 0 or Sc - 1 is outside the interior and gives the
uniform floor); `peaky` (rand ** 16: most bins fall under the `denom < 1e-5` branch).
Draws: `random`; `linspace` (the render's own rows, u = 0 and u = 1 included); `on_cdf` (the restatement's CDF entries, each also one
ulp above and below: the right-sided search); `ties` (rows TIES_EQUAL_ROWS all equal, the others with pairs and triples of equal
values at random places); `outside` (-0.5, 1.5 and -0.0 mixed into random rows)."""
import torch

from pdf_ref import pdf_cdf_ref

GROUPS = {
    "tiny": [(3, 1), (3, 64), (4, 5), (5, 63)],
    "chunk": [(63, 65), (65, 64), (66, 7), (67, 3)],
    "chunks": [(127, 129), (128, 128), (129, 191), (130, 33), (192, 64), (257, 300)],
    "bound": [(200, 824), (960, 64), (1020, 4), (1021, 3), (1023, 1)],
}
SHAPES = [s for g in GROUPS.values() for s in g]
BIG_LDS = [(1021, 3), (1023, 1)]          # > 64 KiB of LDS per workgroup
UNDER_BIG_LDS = (1020, 4)                 # 65344 B
N = 257
NEAR, FAR = 2.0, 6.0
WEIGHTS = ("random", "zero", "onehot", "peaky")
DRAWS = ("random", "linspace", "on_cdf", "ties", "outside")
TIES_EQUAL_ROWS = (0, N - 1)
OUTSIDE = (-0.5, 1.5, -0.0)


def gen_of(Sc, I, salt=0):
    return torch.Generator().manual_seed(Sc * 100003 + I * 101 + salt)


def zgrid_of(Sc):
    return torch.linspace(NEAR, FAR, Sc)


def jitter_of(Sc, gen, n=N):
    return torch.rand(n, generator=gen) * (FAR - NEAR) / Sc


def weights_of(kind, Sc, gen, n=N):
    if kind == "random":
        return torch.rand(n, Sc, generator=gen)
    if kind == "zero":
        return torch.zeros(n, Sc)
    if kind == "onehot":
        pos = torch.randint(0, Sc, (n,), generator=gen)
        pos[0], pos[1] = 0, Sc - 1                                          # both ends are there whatever the draw
        return torch.nn.functional.one_hot(pos, Sc).float()
    if kind == "peaky":
        return torch.rand(n, Sc, generator=gen) ** 16
    raise KeyError(kind)


def draws_of(kind, w, I, gen):
    n, Sc = w.shape
    if kind == "random":
        return torch.rand(n, I, generator=gen)
    if kind == "linspace":
        return torch.linspace(0, 1, I).expand(n, -1).contiguous()
    if kind == "on_cdf":
        cdf = pdf_cdf_ref(w)[1]                                             # [n, Sc-1]
        s = torch.arange(I).unsqueeze(0) + torch.arange(n).unsqueeze(1)     # entry s // 3 exactly, one ulp up, one ulp down
        u = cdf.gather(1, (s // 3) % (Sc - 1))
        up, down = torch.nextafter(u, torch.full_like(u, 2.0)), torch.nextafter(u, torch.full_like(u, -1.0))
        return torch.where(s % 3 == 1, up, torch.where(s % 3 == 2, down, u)).contiguous()
    if kind == "ties":
        u = torch.rand(n, I, generator=gen)
        p = torch.rand(n, I, generator=gen).argsort(1)                      # a random order of the columns, per row
        rows = torch.arange(n)
        if I >= 5:                                                          # a pair and a triple
            u[rows, p[:, 1]] = u[rows, p[:, 0]]
            u[rows, p[:, 3]] = u[rows, p[:, 2]]
            u[rows, p[:, 4]] = u[rows, p[:, 2]]
        elif I >= 2:                                                        # a pair; on odd rows a triple where there is room
            u[rows, p[:, 1]] = u[rows, p[:, 0]]
            if I >= 3:
                odd = rows[rows % 2 == 1]
                u[odd, p[odd, 2]] = u[odd, p[odd, 0]]
        u[TIES_EQUAL_ROWS[0]] = u[TIES_EQUAL_ROWS[0], 0]
        u[TIES_EQUAL_ROWS[1]] = 0.0
        return u
    if kind == "outside":
        u = torch.rand(n, I, generator=gen)
        which = torch.randint(0, 12, (n, I), generator=gen)                 # a quarter of the draws, a twelfth each
        which[torch.arange(n), torch.arange(n) % I] = torch.arange(n) % 4   # ... and in every row with room one of them, or none
        for i, v in enumerate(OUTSIDE):
            u[which == i] = v
        return u
    raise KeyError(kind)


def cases(Sc, I):
    """Yields (name, w [N,Sc], zgrid [Sc], jitter [N] | None, u [N,I]): every weight kind with every draw kind on a jittered grid, and
    per weight kind one pass on the bare grid."""
    gen = gen_of(Sc, I)
    zgrid = zgrid_of(Sc)
    for wi, wk in enumerate(WEIGHTS):
        w = weights_of(wk, Sc, gen)
        jit = jitter_of(Sc, gen)
        for uk in DRAWS:
            yield f"{wk}/{uk}", w, zgrid, jit, draws_of(uk, w, I, gen)
        uk = DRAWS[wi % len(DRAWS)]
        yield f"{wk}/{uk}/bare", w, zgrid, None, draws_of(uk, w, I, gen)


def edges_ref(zgrid, jitter, n=N):
    """The bin edges mid [n, Sc-1] of the contract: zc = zgrid + jitter, mid = 0.5 (zc[i] + zc[i+1]), each operation rounded."""
    zc = zgrid.reshape(1, -1).float() + (torch.zeros(n) if jitter is None else jitter.reshape(n).float()).unsqueeze(1)
    return 0.5 * (zc[:, :-1] + zc[:, 1:])


def same_bits(a, b):
    """torch.equal on the bits: -0.0 and 0.0 differ, a NaN equals itself."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
