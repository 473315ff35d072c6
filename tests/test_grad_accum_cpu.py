"""Gradient accumulation (accum_steps), the host side: the C ABI lists, option validation from the optimizer up to the training driver's
flag, and FusedAdam's micro-step bookkeeping on CPU tensors with hand-set gradients.  No kernel runs here: the Adam launches of a
group's end (FusedAdam._apply) are replaced by a recorder, everything in front of them is the code the GPU path runs."""
import pytest
import torch
import torch.nn as nn

from instancediff_amd import _lib, pipeline, trainUM
from instancediff_amd import train_ops as T
from instancediff_amd.train_ops import FusedAdam

BAD_STEPS = (True, False, 0, -1, 2.0, 1.5, "2", None, [2])
SIZES = (7, 12, 5)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _opt(monkeypatch=None, **kw):
    """three parameters in one group; with monkeypatch the group-end launches are recorded instead of run -> (opt, params, scales)"""
    ps = [nn.Parameter(torch.randn(n, generator=_g(10 + n))) for n in SIZES]
    opt = FusedAdam(ps, lr=1e-3, **kw)
    scales = []
    if monkeypatch is not None:
        monkeypatch.setattr(opt, "_apply", scales.append)
    return opt, ps, scales


def _grads(seed):
    return [torch.randn(n, generator=_g(seed + n)) for n in SIZES]


def _set(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.clone()


def test_entry_point_is_declared_and_bound():
    assert "idiff_gather_segments_acc" in _lib.header_symbols() and "idiff_gather_segments_acc" in _lib.SIGNATURES
    assert _lib.SIGNATURES["idiff_gather_segments_acc"] == _lib.SIGNATURES["idiff_gather_segments"]
    assert sorted(_lib.SIGNATURES) == _lib.header_symbols()


def test_option_parser_and_defaults():
    assert T.parse_accum_steps(1) == 1 and T.parse_accum_steps(7) == 7
    for bad in BAD_STEPS:
        with pytest.raises(ValueError, match="accum_steps"):
            T.parse_accum_steps(bad)
    opt, _, _ = _opt()
    assert opt.accum_steps == 1 and opt.micro_step == 0 and opt.boundary_next is True
    opt, _, _ = _opt(accum_steps=3)
    assert opt.accum_steps == 3 and opt.micro_step == 0 and opt.boundary_next is False
    for bad in BAD_STEPS:
        with pytest.raises(ValueError, match="accum_steps"):
            _opt(accum_steps=bad)
        with pytest.raises(ValueError, match="accum_steps"):
            opt.set_accum_steps(bad)
    assert opt.accum_steps == 3  # a refused call changed nothing
    opt.set_accum_steps(2)
    assert opt.accum_steps == 2


def test_three_micro_steps_sum_in_order_and_apply_once(monkeypatch):
    opt, ps, scales = _opt(monkeypatch, accum_steps=3)
    opt.grad_scale = 0.5
    flat = opt._flat[0]["g"]
    g0, g1, g2 = _grads(100), _grads(200), _grads(300)
    g2[1] = None  # the middle parameter receives no gradient in the third micro-step
    epoch0, step0 = T.WEIGHT_EPOCH[0], opt._flat[0]["step"]
    returned = []
    for i, gs in enumerate((g0, g1, g2)):
        opt.zero_grad()
        _set(ps, gs)
        assert opt.micro_step == i and opt.boundary_next is (i == 2)
        if i == 1:  # flat_grads() twice adds once
            first = opt.flat_grads()[0].clone()
            assert torch.equal(opt.flat_grads()[0], first)
        returned.append(opt.step())
        if i < 2:
            assert scales == [] and T.WEIGHT_EPOCH[0] == epoch0 and opt._flat[0]["step"] == step0
    assert returned == [False, False, True]
    want = torch.cat([(g0[0] + g1[0]) + g2[0], g0[1] + g1[1], (g0[2] + g1[2]) + g2[2]])
    assert torch.equal(flat, want)  # ((g0 + g1) + g2), bit for bit; the parameter without a gradient kept its sum
    assert scales == [0.5 / 3] and opt.micro_step == 0
    for p, o in zip(ps, (0, 7, 19)):
        assert p.grad.data_ptr() == flat.data_ptr() + 4 * o  # the views are bound again
    # the next group starts by assigning: a parameter without a gradient gets zeros
    opt.zero_grad()
    _set(ps, [g1[0], None, g1[2]])
    assert opt.step() is False
    assert torch.equal(flat, torch.cat([g1[0], torch.zeros(12), g1[2]]))


def test_zero_grad_keeps_the_sum_while_a_group_is_open(monkeypatch):
    opt, ps, _ = _opt(monkeypatch, accum_steps=2)
    flat = opt._flat[0]["g"]
    g0 = _grads(400)
    opt.zero_grad()
    _set(ps, g0)
    assert opt.step() is False
    opt.zero_grad(set_to_none=False)  # a group is open: views re-bound, nothing zero-filled
    assert torch.equal(flat, torch.cat(g0))
    assert all(p.grad is not None and p.grad.data_ptr() == flat.data_ptr() + 4 * o for p, o in zip(ps, (0, 7, 19)))
    ps[0].grad.add_(1.0)  # what a backward does to a bound view
    assert opt.step() is True
    assert torch.equal(flat, torch.cat([g0[0] + 1.0, g0[1], g0[2]]))
    opt.zero_grad(set_to_none=False)  # no group open: torch.optim semantics
    assert float(flat.abs().max()) == 0.0


def test_open_group_refuses_state_dict_and_option_change(monkeypatch):
    opt, ps, scales = _opt(monkeypatch, accum_steps=3)
    opt.state_dict()  # nothing held: fine
    _set(ps, _grads(500))
    assert opt.step() is False
    with pytest.raises(RuntimeError, match="group of micro-steps is open"):
        opt.state_dict()
    with pytest.raises(RuntimeError, match="group of micro-steps is open"):
        opt.set_accum_steps(2)
    assert opt.accum_steps == 3 and opt.micro_step == 1
    assert opt.discard_accumulated() == 1 and opt.micro_step == 0 and opt.discard_accumulated() == 0
    assert "flat" in opt.state_dict()
    opt.set_accum_steps(2)
    # the discarded gradient is gone: the next one is assigned, not added
    g = _grads(600)
    opt.zero_grad()
    _set(ps, g)
    assert opt.step() is False
    assert torch.equal(opt._flat[0]["g"], torch.cat(g)) and scales == []


def test_one_step_per_call_by_default(monkeypatch):
    opt, ps, scales = _opt(monkeypatch)
    opt.grad_scale = 0.125
    flat = opt._flat[0]["g"]
    for seed in (700, 800):
        g = _grads(seed)
        g[2] = None
        opt.zero_grad()
        _set(ps, g)
        assert opt.step() is True and opt.micro_step == 0
        assert torch.equal(flat, torch.cat([g[0], g[1], torch.zeros(5)]))  # assigned every time, zeros without a gradient
    assert scales == [0.125, 0.125]  # grad_scale itself
    opt.state_dict()


def test_pipeline_build_refuses_bad_accum_steps():
    cpu = torch.device("cpu")
    for bad in (True, 0, -3, 2.0, "2"):
        with pytest.raises(ValueError, match="accum_steps"):
            pipeline.build(phase="train", device=cpu, T=4, accum_steps=bad)


def test_train_flag_reaches_the_model_option_and_both_optimizers():
    parser = trainUM.build_parser()
    off = parser.parse_args(["-opt", "x.yml"])
    assert off.accum_steps is None
    opt = pipeline.load_options()
    which = opt["train"]["which_model"]
    trainUM.apply_model_overrides(opt, off)
    assert opt["models"][which].get("accum_steps") is None
    model, _ = pipeline.build(opt=opt, phase="train", device=torch.device("cpu"), T=4)
    assert model.accum_steps == 1 and model.stepped is False
    assert model.drift_optimizer.accum_steps == 1 and model.noise_optimizer.accum_steps == 1
    on = parser.parse_args(["-opt", "x.yml", "--accum-steps", "4"])
    trainUM.apply_model_overrides(opt, on)
    assert opt["models"][which]["accum_steps"] == 4
    model, _ = pipeline.build(opt=opt, phase="train", device=torch.device("cpu"), T=4)
    assert model.accum_steps == 4
    for o in (model.drift_optimizer, model.noise_optimizer):
        assert o.accum_steps == 4 and o.boundary_next is False
    model.set_accum_steps(2)
    assert model.accum_steps == 2 and model.drift_optimizer.accum_steps == 2 and model.noise_optimizer.accum_steps == 2
    assert model.discard_accumulated() == 0
    # pipeline.build's own switch overrides the option the same way, and the caller's options are not written to
    model2, _ = pipeline.build(opt=opt, phase="train", device=torch.device("cpu"), T=4, accum_steps=3)
    assert model2.accum_steps == 3 and opt["models"][which]["accum_steps"] == 4
    with pytest.raises(SystemExit):
        parser.parse_args(["-opt", "x.yml", "--accum-steps", "2.5"])
