"""CPU: the model-wide optimiser's host side (nopesac_amd/optim.py, ops.opt_unit_map) - the schedule, the unit map and the kernels' index
arithmetic over it (a wrong table is a GPU fault: proven here before anything runs on a GPU), the grouping against step_from_cfg, the
gradient average over gloo, and the header's new rows."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import model_optimizer_forms as M


# ---------------------------------------------------------------------------------------------------------------------------- lr_at
def test_lr_at_defaults_by_hand():
    """config.py's defaults: BASE_LR 1e-3, linear warm-up from factor 1e-3 over 1000 iterations, x GAMMA 0.1 at STEPS (30000,)."""
    from nopesac_amd.config import get_cfg
    from nopesac_amd.optim import lr_at
    cfg = get_cfg()
    want = {0: 1e-6, 1: 1.999e-6, 500: 5.005e-4, 999: 9.99001e-4, 1000: 1e-3, 29999: 1e-3, 30000: 1e-4, 39999: 1e-4}
    for it, lr in want.items():
        assert lr_at(cfg, it) == pytest.approx(lr, rel=1e-12), it


def test_lr_at_constant_warmup_two_steps_and_refusals():
    from nopesac_amd.config import get_cfg
    from nopesac_amd.optim import lr_at
    cfg = get_cfg()
    cfg.merge_from_list(["SOLVER.WARMUP_METHOD", "constant", "SOLVER.WARMUP_ITERS", 10, "SOLVER.WARMUP_FACTOR", 0.25, "SOLVER.BASE_LR", 0.02,
                         "SOLVER.STEPS", (20, 30), "SOLVER.GAMMA", 0.5])
    want = {0: 0.005, 9: 0.005, 10: 0.02, 19: 0.02, 20: 0.01, 29: 0.01, 30: 0.005, 1000: 0.005}
    for it, lr in want.items():
        assert lr_at(cfg, it) == pytest.approx(lr, rel=1e-12), it
    cfg.merge_from_list(["SOLVER.WARMUP_METHOD", "burnin"])
    with pytest.raises(NotImplementedError, match="WARMUP_METHOD"):
        lr_at(cfg, 0)
    cfg.merge_from_list(["SOLVER.WARMUP_METHOD", "linear", "SOLVER.LR_SCHEDULER_NAME", "WarmupCosineLR"])
    with pytest.raises(NotImplementedError, match="LR_SCHEDULER_NAME"):
        lr_at(cfg, 0)


# ---------------------------------------------------------------------------------------------------------------------------- unit map
def _check_map(sizes):
    from nopesac_amd import ops
    offsets, units, arena = ops.opt_unit_map(sizes)
    sizes = np.asarray(sizes, dtype=np.int64)
    assert (offsets % M.ALIGN == 0).all() and arena % M.ALIGN == 0
    ends = offsets + sizes
    assert (ends[:-1] <= offsets[1:]).all() and ends[-1] <= arena                    # no overlap, everything inside the arena
    assert (offsets[1:] - ends[:-1] < M.ALIGN).all() and arena - ends[-1] < M.ALIGN   # and no more padding than the alignment asks
    assert units.dtype == np.int32 and units.shape == (int(((sizes + M.CHUNK - 1) // M.CHUNK).sum()), 2)
    seg, chunk = units[:, 0].astype(np.int64), units[:, 1].astype(np.int64)
    assert (seg >= 0).all() and (seg < len(sizes)).all() and (np.diff(seg) >= 0).all()
    lo = chunk * M.CHUNK
    hi = np.minimum(lo + M.CHUNK, sizes[seg])
    assert (lo < sizes[seg]).all() and (hi <= sizes[seg]).all()                       # no unit crosses its segment's end
    covered = [np.zeros(int(n), np.int32) for n in sizes]
    for s, a, b in zip(seg.tolist(), lo.tolist(), hi.tolist()):
        covered[s][a:b] += 1
    assert all((c == 1).all() for c in covered)                                       # every element exactly once
    return offsets, units, arena


def _check_emulation(sizes, offsets, units, arena, aligned, present):
    stores, ok = M.emulate_step(sizes, offsets, units, arena, aligned)
    assert ok, "a clamped load of the step kernel leaves its segment"
    assert all((c == 1).all() for c in stores), "the step kernel does not store every live element exactly once"
    touched, ok = M.emulate_gather(sizes, offsets, units, arena, aligned, present)
    assert ok, "a clamped load of the gather kernel leaves its source"
    live = np.zeros(arena, bool)
    for o, n in zip(np.asarray(offsets).tolist(), list(sizes)):
        live[o:o + n] = True
        assert (touched[o + n:o + (n + 3) // 4 * 4] <= 1).all()                       # the last vector's zero lanes: the segment's own padding
        assert (touched[o + (n + 3) // 4 * 4:(o + n + M.ALIGN - 1) // M.ALIGN * M.ALIGN] == 0).all()
    assert (touched[live] == 1).all(), "the gather does not write every live float exactly once"


def test_unit_map_boundary_sizes():
    from nopesac_amd import ops
    sizes = list(M.SIZES)
    offsets, units, arena = _check_map(sizes)
    for aligned, present in ((True, True), (False, True), (True, False)):
        _check_emulation(sizes, offsets, units, arena, [aligned] * len(sizes), [present] * len(sizes))
    mixed = [i % 2 == 0 for i in range(len(sizes))]
    _check_emulation(sizes, offsets, units, arena, mixed, [i % 3 != 0 for i in range(len(sizes))])
    for n in M.SIZES:                                                                  # each size alone, and first / last in a pair
        _check_map([n])
        _check_map([n, 5])
        _check_map([5, n])
    for bad in ([], [0], [4, -1]):
        with pytest.raises(ops.OpsArgumentError):
            ops.opt_unit_map(bad)


def test_unit_map_of_the_real_model():
    """The 652 tensors / 75.3 M floats of the seven trainers on the synthetic checkpoint."""
    sizes = M.real_sizes()
    assert len(sizes) == 652 and 75.2e6 < sum(sizes) < 75.4e6 and min(sizes) == 1
    offsets, units, arena = _check_map(sizes)
    stores, ok = M.emulate_step(sizes, offsets, units, arena, [i % 5 != 0 for i in range(len(sizes))])
    assert ok and all((c == 1).all() for c in stores)


def test_gather_addressing_of_the_real_model():
    from nopesac_amd import ops
    sizes = M.real_sizes()
    offsets, units, arena = ops.opt_unit_map(sizes)
    touched, ok = M.emulate_gather(sizes, offsets, units, arena, [i % 5 != 0 for i in range(len(sizes))], [i % 7 != 0 for i in range(len(sizes))])
    live = np.zeros(arena, bool)
    for o, n in zip(offsets.tolist(), sizes):
        live[o:o + n] = True
    assert ok and (touched[live] == 1).all() and touched.max() == 1
    assert int(touched.sum()) <= sum((n + 3) // 4 * 4 for n in sizes)                 # beyond the live floats only last-vector lanes


def test_emulation_notices_a_wrong_map():
    """The restatement is a check, not a tautology: a unit past its segment's end is dropped (the kernel skips it), a missing or a
    doubled unit shows in the counts."""
    from nopesac_amd import ops
    sizes = [4097, 3]
    offsets, units, arena = ops.opt_unit_map(sizes)
    for wrong in (units[:-1], np.concatenate([units, units[:1]]), np.concatenate([units[:1], units[2:]])):
        stores, _ = M.emulate_step(sizes, offsets, wrong, arena, [True, True])
        assert not all((c == 1).all() for c in stores)
    stores, ok = M.emulate_step(sizes, offsets, np.array([[0, 0], [0, 1], [0, 2], [1, 0], [2, 0], [-1, 0]], np.int32), arena, [True, True])
    assert ok and all((c == 1).all() for c in stores)                                  # out-of-table units touch nothing


# ---------------------------------------------------------------------------------------------------------------------------- grouping
def _toy_trainers():
    Head, Backbone = M.toy_classes()
    a = Head({M.key_for(i): torch.zeros(n) for i, n in enumerate((3, 5, 7))})
    b = Backbone({"backbone." + M.key_for(i): torch.zeros(2) for i in range(3)})
    return a, b


@pytest.mark.parametrize("name", ["ADAMW", "SGD"])
def test_groups_are_what_step_from_cfg_passes(name, monkeypatch):
    from nopesac_amd import optim, training
    cfg = M.solver_cfg("SOLVER.OPTIMIZER", name)
    trainers = _toy_trainers()
    keys, params, index, groups = optim.parameter_table(trainers, cfg, weight_decay=float(cfg.SOLVER.WEIGHT_DECAY),
                                                        weight_decay_norm=float(cfg.SOLVER.WEIGHT_DECAY_NORM),
                                                        weight_decay_embed=float(cfg.SOLVER.WEIGHT_DECAY_EMBED))
    assert keys == [k for tr in trainers for k in tr.params]
    assert all(a is b for a, b in zip(params, [p for tr in trainers for p in tr.params.values()]))
    assert {training.parameter_group(k) for k in trainers[0].params} == {"plain", "norm", "embed"}
    assert len(groups) == 4 and len(set(groups)) == 4                                  # three decays at multiplier 1; "backbone." keys are all plain
    seen = {}

    def recording_step(self, lr=1e-4, optimizer="ADAMW", weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8, momentum=0.9, weight_decay_norm=None,
                       weight_decay_embed=None):
        for k in self.params:
            seen[k] = (lr, self._weight_decay(k, weight_decay, weight_decay_norm, weight_decay_embed), optimizer, momentum)
    monkeypatch.setattr(training.HeadTrainer, "step", recording_step)
    for tr in trainers:
        tr.step_from_cfg(cfg)
    base = float(cfg.SOLVER.BASE_LR)
    for k, g in zip(keys, index):
        mult, wd = groups[g]
        assert (base * mult, wd) == seen[k][:2], k                                     # the same doubles: the same f32 after one rounding
        assert seen[k][2] == name and seen[k][3] == float(cfg.SOLVER.MOMENTUM)
    assert {groups[g][0] for k, g in zip(keys, index) if k.startswith("backbone.")} == {0.1}


def test_seventeenth_group_and_duplicate_key_raise():
    from nopesac_amd import optim, training
    Head, _ = M.toy_classes()
    cfg = M.solver_cfg()

    def with_multiplier(m, i):
        cls = type("Toy%d" % i, (Head,), {"lr_multiplier": lambda self, cfg, m=m: m})
        return cls({"toy%d.w" % i: torch.zeros(2)})
    sixteen = [with_multiplier(1.0 + i, i) for i in range(16)]
    assert len(optim.parameter_table(sixteen, cfg)[3]) == 16
    with pytest.raises(ValueError, match="more than 16"):
        optim.parameter_table(sixteen + [with_multiplier(99.0, 16)], cfg)
    a, b = _toy_trainers()
    twin = Head({M.key_for(0): torch.zeros(3)})
    with pytest.raises(ValueError, match="held by two trainers"):
        optim.parameter_table([a, b, twin], cfg)
    with pytest.raises(ValueError, match="held by two trainers"):                      # raised before any device is asked for
        optim.ModelOptimizer.from_cfg([a, twin], cfg)
    sd_keys = ["camera_head_list.0.geo_encoder.0.weight", "camera_head_list.0.fc_trans.weight"]
    assert set(training.RefineTrainer.parameter_names(sd_keys)) < set(training.CameraHeadTrainer.parameter_names(sd_keys))
    with pytest.raises(ValueError, match="contiguous f32 tensors on one GPU"):         # host parameters never reach a table
        optim.ModelOptimizer.from_cfg([a], cfg)
    cfg.merge_from_list(["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "value"])
    with pytest.raises(NotImplementedError, match="CLIP_TYPE"):
        optim.ModelOptimizer.from_cfg([a], cfg)


# ---------------------------------------------------------------------------------------------------------------------------- average_across_ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_buffer(rank, n=1000):
    return torch.arange(n, dtype=torch.float32) * (rank + 1) + rank


def _average_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from nopesac_amd import optim, runner
    runner.init_distributed("gloo")
    flat = _rank_buffer(rank)
    out = optim.average_across_ranks(flat)
    torch.distributed.barrier()
    q.put((rank, flat.numpy().copy(), out.data_ptr() == flat.data_ptr()))
    torch.distributed.destroy_process_group()


def test_average_across_ranks_world2():
    from nopesac_amd import optim
    flat = _rank_buffer(0)
    assert optim.average_across_ranks(flat) is flat and torch.equal(flat, _rank_buffer(0))      # no process group: nothing happens
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_average_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    mean = ((_rank_buffer(0) + _rank_buffer(1)) / 2).numpy()
    for rank, flat, in_place in got:
        assert in_place and np.array_equal(flat, mean), rank


# ---------------------------------------------------------------------------------------------------------------------------- header
def test_header_rows_of_the_model_optimizer():
    import ctypes
    from nopesac_amd import _lib, ops
    assert (_lib.H.NPS_OPT_CHUNK, _lib.H.NPS_OPT_ALIGN, _lib.H.NPS_OPT_MAX_GROUPS, _lib.H.NPS_OPT_MAX_SEGMENTS) == (4096, 64, 16, 65536)
    assert (ops.OPT_CHUNK, ops.OPT_ALIGN, ops.OPT_MAX_GROUPS, ops.OPT_MAX_SEGMENTS) == (
        _lib.H.NPS_OPT_CHUNK, _lib.H.NPS_OPT_ALIGN, _lib.H.NPS_OPT_MAX_GROUPS, _lib.H.NPS_OPT_MAX_SEGMENTS)
    assert (M.CHUNK, M.ALIGN) == (ops.OPT_CHUNK, ops.OPT_ALIGN)
    assert (ops.OPT_PRESENT, ops.OPT_FIRST) == (_lib.H.NPS_OPT_PRESENT, _lib.H.NPS_OPT_FIRST) == (1, 2)
    assert ops.OPT_MODES == {"ADAMW": _lib.H.NPS_OPT_ADAMW, "SGD": _lib.H.NPS_OPT_SGD}
    assert {"nopesac_opt_gather", "nopesac_opt_step"} <= _lib.STATUS
    assert (ctypes.sizeof(_lib.OptSegment), ctypes.sizeof(_lib.OptSource), ctypes.sizeof(_lib.OptUnit)) == (32, 16, 8)
    assert [(n, getattr(_lib.OptSegment, n).offset) for n, _ in _lib.OptSegment._fields_] == [("param", 0), ("offset", 8), ("n", 16), ("group", 24), ("reserved", 28)]
    assert _lib.OptStepArgs.groups.size == 16 * 8 and ctypes.sizeof(_lib.OptStepArgs) == 232


def test_launchers_refuse_bad_scalars_without_a_gpu():
    """Every scalar of the two entries is checked before any HIP call: NPS_E_ARG and a message, on a machine without a GPU too."""
    import ctypes
    from nopesac_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    tbl = ctypes.cast(buf, ctypes.c_void_p)

    def args(**kw):
        a = _lib.OptStepArgs()
        a.segments = a.sources = a.units = a.G = a.M1 = a.M2 = tbl
        a.n_units, a.arena_floats, a.n_segments, a.mode, a.n_groups, a.step = 1, 64, 1, _lib.H.NPS_OPT_ADAMW, 1, 1
        a.beta1, a.beta2, a.eps, a.momentum = 0.9, 0.999, 1e-8, 0.9
        a.groups[0].lr, a.groups[0].weight_decay = 0.1, 0.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    bad = (dict(segments=None), dict(n_segments=0), dict(n_segments=_lib.H.NPS_OPT_MAX_SEGMENTS + 1), dict(n_units=0), dict(n_units=2),
           dict(arena_floats=63), dict(arena_floats=0), dict(mode=2), dict(G=None), dict(M1=None), dict(M2=None), dict(n_groups=0), dict(n_groups=17),
           dict(step=0), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=float("nan")), dict(mode=_lib.H.NPS_OPT_SGD, momentum=-1.0))
    for kw in bad:
        assert lib.nopesac_opt_step(ctypes.byref(args(**kw)), None) == _lib.H.NPS_E_ARG, kw
        assert lib.nopesac_last_error().startswith(b"opt_step: "), kw
    a = args()
    a.groups[0].lr = float("inf")
    assert lib.nopesac_opt_step(ctypes.byref(a), None) == _lib.H.NPS_E_ARG
    assert lib.nopesac_opt_step(None, None) == _lib.H.NPS_E_ARG
    for kw in (dict(n_segments=0), dict(n_units=0), dict(arena_floats=32), dict(G=None), dict(segments=None)):
        p = dict(segments=tbl, sources=tbl, units=tbl, n_segments=1, n_units=1, G=tbl, arena_floats=64)
        p.update(kw)
        assert lib.nopesac_opt_gather(p["segments"], p["sources"], p["units"], p["n_segments"], p["n_units"], p["G"], p["arena_floats"], None) == _lib.H.NPS_E_ARG, kw
        assert lib.nopesac_last_error().startswith(b"opt_gather: "), kw
