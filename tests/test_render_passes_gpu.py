"""The render pipeline as the kernels and the allocator see it, through the public API only (NeRF_Model.render_rays_train /
render_rays_test / inference, the workspace pool) plus a wrapper around `mc_nerf_amd._lib.call`: which entry points a train step, a
render and a structured `inference` launch and in which order, how many device allocations a steady-state train step makes, that
the train, only-coarse and test spellings of a pass compute the same bits, and that a forward that raises leaves the workspace pool
as it found it.  Small nets and few rays: these are host-side properties, the kernels' numerics have their own tests."""
import pytest
import torch

from mc_nerf_amd import synthetic as S

pytestmark = pytest.mark.gpu

N_RAYS = 256
VOXEL = dict(coarse_sampler="voxel", grid_nerf=16, voxel_warmup_epoch=5)
# name -> (sys_param keys, cur_epoch of the train call, only_coarse)
MODES = {
    "uncapped": (dict(samples=32, scale=2), 0, False),                       # 64 <= 128 fine samples per ray: the cap cannot bind
    "capped": (dict(samples=32, scale=5), 0, False),                         # 160 > 128: the cap path
    "pdf": (dict(samples=32, scale=2, fine_sampler="pdf", n_importance=32), 0, False),
    "voxel_warmup": (dict(samples=32, scale=2, **VOXEL), 0, False),          # cur_epoch below the warm-up: dense coarse pass
    "voxel_pruned": (dict(samples=32, scale=2, **VOXEL), 5, False),          # past it: the grid's list
    "only_coarse": (dict(samples=32, scale=2), 0, True),
}
PRECISIONS = ("f32", "f16x3")          # the two entry-point families: mcnerf_mlp_* and mcnerf_mlp_*_16
CASES = [(mode, precision) for mode in MODES for precision in PRECISIONS]


def _model(dev, mode, precision, n_rays=N_RAYS):
    from mc_nerf_amd.model import NeRF_Model
    torch.manual_seed(1)               # (identical parameters in every model of one mode and precision)
    sp = S.make_sys_param(dev, batch=n_rays, H=32, W=32, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision=precision, **MODES[mode][0])
    return NeRF_Model(sp).to(dev)


def _rays(dev, n_rays=N_RAYS):
    g = torch.Generator().manual_seed(2)
    o = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1) * 3.0
    d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(n_rays, 3, generator=g), dim=-1)
    return d.to(dev), o.to(dev)


def _draws(m, dev, n_rays=N_RAYS, jitter=True):
    """Every draw of a render as an injected tensor (train and test calls then see the same ones)."""
    g = torch.Generator().manual_seed(3)
    st = m.settings
    s_f = st.samples_pdf if st.pdf else st.samples_f
    dr = dict(eps_c=torch.randn(n_rays, st.samples_c, generator=g), eps_sel=torch.randn(n_rays, st.samples_c, generator=g),
              eps_f=torch.randn(n_rays, s_f, generator=g), jitter=torch.rand(n_rays, 1, generator=g) * ((m.far - m.near) / st.samples_c))
    if st.pdf:
        dr["u"] = torch.rand(n_rays, st.n_importance, generator=g)
    if not jitter:
        dr["jitter"] = torch.zeros(n_rays, 1)
    return {k: v.to(dev) for k, v in dr.items()}


def _train(m, mode, d, o, **draws):
    """One train call of the mode -> (rgb_c, rgb_f | None)."""
    _, cur_epoch, only_coarse = MODES[mode]
    out = m.render_rays_train(d, o, cur_epoch, 1.0, only_coarse=only_coarse, **draws)
    return out[0], out[1]


def _step(m, mode, d, o, **draws):
    rgb_c, rgb_f = _train(m, mode, d, o, **draws)
    m.zero_grad(set_to_none=True)
    (rgb_c.sum() if rgb_f is None else rgb_c.sum() + rgb_f.sum()).backward()


# ---------------------------------------------------------------------------------------------------------------- launch sequence
# Entry points without the "mcnerf_" prefix; "*" is "" in f32 and "_16" in the register-chain modes.
TRAIN = {
    "uncapped": ["upload_f32", "pack_weights*", "mlp_fwd*", "composite_fwd",
                 "pack_weights*", "select_fine", "mlp_fwd*", "composite_fwd",
                 "composite_bwd", "mlp_bwd*", "mlp_dw*", "composite_bwd", "mlp_bwd*", "mlp_dw*"],
    "capped": ["upload_f32", "pack_weights*", "mlp_fwd*", "composite_fwd",
               "pack_weights*", "select_fine", "cap_random", "mlp_fwd*", "composite_fwd",
               "composite_bwd", "mlp_bwd*", "mlp_dw*", "composite_bwd", "mlp_bwd*", "mlp_dw*"],
    "pdf": ["upload_f32", "pack_weights*", "mlp_fwd*", "composite_fwd",
            "pack_weights*", "sample_pdf", "mlp_fwd*", "composite_fwd",
            "composite_bwd", "mlp_bwd*", "mlp_dw*", "composite_bwd", "mlp_bwd*", "mlp_dw*"],
    "voxel_warmup": ["upload_f32", "pack_weights*", "mlp_fwd*", "composite_fwd", "voxel_update",
                     "pack_weights*", "select_fine", "mlp_fwd*", "composite_fwd",
                     "composite_bwd", "mlp_bwd*", "mlp_dw*", "composite_bwd", "mlp_bwd*", "mlp_dw*"],
    "voxel_pruned": ["upload_f32", "pack_weights*", "voxel_select", "mlp_fwd*", "composite_fwd", "voxel_update",
                     "pack_weights*", "select_fine", "mlp_fwd*", "composite_fwd",
                     "composite_bwd", "mlp_bwd*", "mlp_dw*", "composite_bwd", "mlp_bwd*", "mlp_dw*"],
    "only_coarse": ["upload_f32", "pack_weights*", "mlp_fwd*", "composite_fwd",
                    "composite_bwd", "mlp_bwd*", "mlp_dw*"],
}
RENDER = {          # render_rays_test: both nets' weights and the BARF weights first; never a cap, never a grid update
    "threshold": ["pack_weights*", "pack_weights*", "upload_f32", "mlp_fwd*", "composite_fwd", "select_fine", "mlp_fwd*", "composite_fwd"],
    "pdf": ["pack_weights*", "pack_weights*", "upload_f32", "mlp_fwd*", "composite_fwd", "sample_pdf", "mlp_fwd*", "composite_fwd"],
    "voxel": ["pack_weights*", "pack_weights*", "upload_f32", "voxel_select", "mlp_fwd*", "composite_fwd",
              "select_fine", "mlp_fwd*", "composite_fwd"],
}
RENDER_OF = {"uncapped": "threshold", "capped": "threshold", "pdf": "pdf", "voxel_warmup": "voxel", "voxel_pruned": "voxel",
             "only_coarse": "threshold"}
INFERENCE = ["pack_weights*", "upload_f32", "mlp_fwd*", "composite_fwd"]          # with and without idx_render


def _names(lst, precision):
    return ["mcnerf_" + n.replace("*", "" if precision == "f32" else "_16") for n in lst]


@pytest.mark.parametrize("mode,precision,n_rays", [(m, p, N_RAYS) for m, p in CASES] + [("uncapped", "f16x3", 63)])
def test_launch_sequence_of_train_render_and_inference(gpu_device, monkeypatch, mode, precision, n_rays):
    """The entry points of one train step (forward and backward), one render and one structured `inference` with and without an index
    list, in launch order, against the lists above (written from the pipeline as it was spelt out in RenderTrainFn.forward / backward,
    render_test and NeRF_Model._inference before they shared one pass description)."""
    from mc_nerf_amd import _lib
    dev = gpu_device
    m = _model(dev, mode, precision, n_rays)
    d, o = _rays(dev, n_rays)
    dr = _draws(m, dev, n_rays)
    _step(m, mode, d, o, **dr)          # (a model's first call also lays out its flat parameter buffers: mcnerf_param_offsets)
    seen = []
    real = _lib.call

    def recording(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", recording)

    def launched(fn):
        del seen[:]
        fn()
        return list(seen)
    assert launched(lambda: _step(m, mode, d, o, **dr)) == _names(TRAIN[mode], precision)
    test_draws = {k: v for k, v in dr.items() if k != "jitter"}
    assert launched(lambda: m.render_rays_test(d, o, m.nerf_coarse, m.nerf_fine, **test_draws)) == _names(RENDER[RENDER_OF[mode]], precision)
    z_vals = m.z_vals_c.unsqueeze(0) + dr["jitter"]
    xyz = o.unsqueeze(1) + d.unsqueeze(1) * z_vals.unsqueeze(-1)
    idx_render = torch.nonzero(dr["eps_c"] > 0.5)
    with torch.no_grad():
        for idx in (None, idx_render):
            got = launched(lambda: m.inference(m.nerf_coarse, m.emmbedding_xyz, 1.0, xyz, d, z_vals, idx_render=idx, eps=dr["eps_c"]))
            assert got == _names(INFERENCE, precision)


# ---------------------------------------------------------------------------------------------------------------- allocator traffic
# Device allocations (torch.cuda.memory_stats: "allocation.all.allocated") of ONE steady-state train step with default draws: forward
# and backward, workspaces reserved, after two warm-up steps.  Measured with this file on the commit before the passes shared one
# description (profiles/render_passes_ab.txt); a step may make fewer, never more.
STEP_ALLOCATIONS = {
    ("uncapped", "f32"): 29, ("uncapped", "f16x3"): 29,
    ("capped", "f32"): 33, ("capped", "f16x3"): 33,
    ("pdf", "f32"): 27, ("pdf", "f16x3"): 27,
    ("voxel_warmup", "f32"): 29, ("voxel_warmup", "f16x3"): 29,
    ("voxel_pruned", "f32"): 33, ("voxel_pruned", "f16x3"): 33,
    ("only_coarse", "f32"): 15, ("only_coarse", "f16x3"): 15,
}


@pytest.mark.parametrize("mode,precision", CASES)
def test_a_train_step_allocates_no_more_than_before(gpu_device, mode, precision):
    dev = gpu_device
    m = _model(dev, mode, precision)
    d, o = _rays(dev)
    m.reserve_workspaces(N_RAYS)
    for _ in range(2):
        _step(m, mode, d, o)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    _step(m, mode, d, o)
    made = torch.cuda.memory_stats(dev)["allocation.all.allocated"] - before
    assert made <= STEP_ALLOCATIONS[(mode, precision)]


# ---------------------------------------------------------------------------------------------------------------- one pass, three spellings
@pytest.mark.parametrize("mode,precision", [c for c in CASES if c[0] != "only_coarse"])
def test_coarse_colour_is_the_same_bits_with_and_without_the_fine_pass(gpu_device, mode, precision):
    """rgb_c of a whole train call and of an only_coarse call: same parameters, same draws, the same coarse pass."""
    dev = gpu_device
    d, o = _rays(dev)
    cur_epoch = MODES[mode][1]
    whole, alone = _model(dev, mode, precision), _model(dev, mode, precision)           # (a train call changes the voxel grid: one model each)
    dr = _draws(whole, dev)
    with torch.no_grad():
        rgb_c = whole.render_rays_train(d, o, cur_epoch, 1.0, **dr)[0]
        rgb_c_alone = alone.render_rays_train(d, o, cur_epoch, 1.0, only_coarse=True, **dr)[0]
    assert torch.isfinite(rgb_c).all() and torch.equal(rgb_c, rgb_c_alone)


# (not "capped": the train call's cap can bind, a render has none.  "voxel_warmup": the train call runs the dense coarse pass, the
# render the list of a fresh grid, which holds sigma_init > voxel_thresh in every cell: every sample, so the same pass)
@pytest.mark.parametrize("mode,precision", [c for c in CASES if c[0] in ("uncapped", "pdf", "voxel_pruned", "voxel_warmup")])
def test_render_is_the_same_bits_as_a_train_call_without_jitter(gpu_device, mode, precision):
    """Jitter 0 and step_r = 1: render_rays_test's rgb is the train call's rgb_f wherever the cap cannot bind."""
    dev = gpu_device
    d, o = _rays(dev)
    train, test = _model(dev, mode, precision), _model(dev, mode, precision)
    dr = _draws(train, dev, jitter=False)
    with torch.no_grad():
        rgb_f = train.render_rays_train(d, o, MODES[mode][1], 1.0, **dr)[1]
        rgb = test.render_rays_test(d, o, test.nerf_coarse, test.nerf_fine, **{k: v for k, v in dr.items() if k != "jitter"})[0]
    assert torch.isfinite(rgb).all() and torch.equal(rgb, rgb_f)


# ---------------------------------------------------------------------------------------------------------------- a failing forward
FAILURES = {        # name -> (mode, the op that raises, on which of its calls in the forward)
    "coarse mlp_fwd": ("uncapped", "mlp_fwd", 1),
    "fine mlp_fwd": ("uncapped", "mlp_fwd", 2),
    "fine composite_fwd": ("uncapped", "composite_fwd", 2),
    "sample_pdf": ("pdf", "sample_pdf", 1),
    "select_fine": ("uncapped", "select_fine", 1),
}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("failure", list(FAILURES))
def test_a_failing_forward_returns_its_workspaces(gpu_device, monkeypatch, failure, precision):
    """A forward that raises anywhere (here: a Python exception from the named op) holds no saved-operand set afterwards: the pool has
    what it had before the call, and the next step re-uses the same buffers instead of allocating another set."""
    from mc_nerf_amd import ops
    from mc_nerf_amd._lib import McnerfError
    mode, op, nth = FAILURES[failure]
    dev = gpu_device
    m = _model(dev, mode, precision)
    d, o = _rays(dev)
    pool_size = lambda: sum(len(v) for v in m.ws_pool.free.values())
    saved_ptrs = lambda: sorted(ws.act.data_ptr() for key, lst in m.ws_pool.free.items() if key[0] == "save" for ws in lst)
    _step(m, mode, d, o)
    n0, ptrs0 = pool_size(), saved_ptrs()
    assert n0 == 4 and len(ptrs0) == 2                                   # (save + grad) x (coarse, fine)
    real, calls = getattr(ops, op), []

    def failing(*a, **kw):
        calls.append(1)
        if len(calls) == nth:
            raise McnerfError("injected failure")
        return real(*a, **kw)
    monkeypatch.setattr(ops, op, failing)
    with pytest.raises(McnerfError, match="injected"):
        _train(m, mode, d, o)
    monkeypatch.setattr(ops, op, real)
    assert len(calls) == nth and pool_size() == n0 and saved_ptrs() == ptrs0
    _step(m, mode, d, o)
    assert pool_size() == n0 and saved_ptrs() == ptrs0


# ---------------------------------------------------------------------------------------------------------------- a forward without a backward
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_forward_without_a_backward_frees_its_workspaces_with_the_graph(gpu_device, precision):
    """A forward whose backward never runs keeps its saved-operand sets (render.WorkspacePool); they must die with the graph, by
    reference count: a full-size set is tens of GB, and a run of such forwards cannot wait for the cycle collector (disabled here)."""
    import gc
    dev = gpu_device
    m = _model(dev, "uncapped", precision)
    d, o = _rays(dev)
    _step(m, "uncapped", d, o)
    pool_size = lambda: sum(len(v) for v in m.ws_pool.free.values())
    n0 = pool_size()
    smallest_set = min(ws.act.numel() * ws.act.element_size() for key, lst in m.ws_pool.free.items() if key[0] == "save" for ws in lst)
    gc.collect()
    gc.disable()
    try:
        held = _train(m, "uncapped", d, o)                               # takes both pooled save sets ...
        before = torch.cuda.memory_allocated(dev)
        second = _train(m, "uncapped", d, o)                             # ... so this one allocates two of its own
        assert pool_size() == n0 - 2 and torch.cuda.memory_allocated(dev) - before > smallest_set
        del second
        # the second forward's sets are gone (what may stay is far smaller: the model's last_selection, now the second call's list)
        assert torch.cuda.memory_allocated(dev) - before < smallest_set
        del held
        assert pool_size() == n0 - 2                                     # (dropped, not returned: the pool re-allocates on demand)
    finally:
        gc.enable()
