"""Gradient guard (global-norm clipping, skipping non-finite steps), the host side: the C ABI lists, option validation from the optimizer
up to the training driver's flags, and FusedAdam's step-count / state-dict bookkeeping on CPU tensors (no kernel runs here)."""
import math

import pytest
import torch
import torch.nn as nn

from instancediff_amd import _lib, pipeline, trainUM
from instancediff_amd.train_ops import FusedAdam, parse_max_grad_norm, parse_skip_nonfinite

BAD_NORMS = (True, False, "1.0", 0, 0.0, -1, -0.5, math.nan, math.inf, -math.inf, [1.0])
BAD_FLAGS = (0, 1, None, "true", 1.0)


def _opt(**kw):
    return FusedAdam(nn.Linear(3, 2).parameters(), lr=1e-3, **kw)


def test_entry_points_are_declared_and_bound():
    for s in ("idiff_grad_sumsq_parts", "idiff_grad_sumsq", "idiff_grad_guard", "idiff_adam_step_dev"):
        assert s in _lib.header_symbols() and s in _lib.SIGNATURES, s
    assert sorted(_lib.SIGNATURES) == _lib.header_symbols()


def test_option_parsers():
    assert parse_max_grad_norm(None) is None
    assert parse_max_grad_norm(2) == 2.0 and isinstance(parse_max_grad_norm(2), float)
    assert parse_max_grad_norm(1e-3) == 1e-3
    for bad in BAD_NORMS:
        with pytest.raises(ValueError, match="max_grad_norm"):
            parse_max_grad_norm(bad)
    assert parse_skip_nonfinite(True) is True and parse_skip_nonfinite(False) is False
    for bad in BAD_FLAGS:
        with pytest.raises(ValueError, match="skip_nonfinite"):
            parse_skip_nonfinite(bad)


def test_fused_adam_validates_the_guard_options():
    opt = _opt()
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False and not opt.guarded
    assert opt.last_info is None and opt.skipped_steps == 0
    opt = _opt(max_grad_norm=3, skip_nonfinite=True)
    assert opt.max_grad_norm == 3.0 and opt.skip_nonfinite is True and opt.guarded
    for bad in BAD_NORMS:
        with pytest.raises(ValueError):
            _opt(max_grad_norm=bad)
        with pytest.raises(ValueError):
            opt.set_grad_guard(max_grad_norm=bad)
    for bad in BAD_FLAGS:
        with pytest.raises(ValueError):
            _opt(skip_nonfinite=bad)
        with pytest.raises(ValueError):
            opt.set_grad_guard(skip_nonfinite=bad)
    assert opt.max_grad_norm == 3.0 and opt.skip_nonfinite is True  # a refused call changed nothing
    opt.set_grad_guard(max_grad_norm=0.5)
    assert opt.max_grad_norm == 0.5 and opt.skip_nonfinite is False and opt.guarded
    opt.set_grad_guard(skip_nonfinite=True)
    assert opt.max_grad_norm is None and opt.guarded
    opt.set_grad_guard()
    assert not opt.guarded


def test_pipeline_build_refuses_bad_guard_options():
    cpu = torch.device("cpu")
    for bad in (True, "1", 0, -2.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="grad_clip_norm"):
            pipeline.build(phase="train", device=cpu, T=4, grad_clip_norm=bad)
    for bad in (1, "yes", 0.0):
        with pytest.raises(ValueError, match="skip_nonfinite_steps"):
            pipeline.build(phase="train", device=cpu, T=4, skip_nonfinite_steps=bad)


def test_train_flags_reach_the_model_options_and_both_optimizers():
    parser = trainUM.build_parser()
    off = parser.parse_args(["-opt", "x.yml"])
    assert off.grad_clip_norm is None and off.skip_nonfinite_steps is False
    opt = pipeline.load_options()
    which = opt["train"]["which_model"]
    trainUM.apply_model_overrides(opt, off)
    assert opt["models"][which].get("grad_clip_norm") is None and opt["models"][which].get("skip_nonfinite_steps") is None
    on = parser.parse_args(["-opt", "x.yml", "--grad-clip-norm", "2.5", "--skip-nonfinite-steps"])
    trainUM.apply_model_overrides(opt, on)
    assert opt["models"][which]["grad_clip_norm"] == 2.5 and opt["models"][which]["skip_nonfinite_steps"] is True
    model, _ = pipeline.build(opt=opt, phase="train", device=torch.device("cpu"), T=4)
    assert model.grad_clip_norm == 2.5 and model.skip_nonfinite_steps is True
    for o in (model.drift_optimizer, model.noise_optimizer):
        assert o.max_grad_norm == 2.5 and o.skip_nonfinite is True
    assert model.grad_info is None and model.get_grad_message() == ""
    model.grad_info = {"drift": {"norm": 3.0, "coef": 0.5, "skipped": False}, "noise": {"norm": 0.25, "coef": 1.0, "skipped": False},
                       "skipped_steps": 2}
    msg = model.get_grad_message()
    assert "3.0000e+00" in msg and "0.5000" in msg and "2.5000e-01" in msg and "1.0000" in msg and "skipped=2" in msg
    # pipeline.build's own switches override the options the same way
    model2, _ = pipeline.build(opt=opt, phase="test", device=torch.device("cpu"), T=4, grad_clip_norm=7, skip_nonfinite_steps=False)
    assert model2.grad_clip_norm == 7.0 and model2.skip_nonfinite_steps is False
    assert opt["models"][which]["grad_clip_norm"] == 2.5  # the caller's options are not written to


def test_settle_and_state_dict_carry_the_skip_count():
    opt = _opt(max_grad_norm=1.0, skip_nonfinite=True)
    f = opt._flat[0]
    f["step"] = 3
    assert opt.settle([0.7, 1.0, 1.0, 0.0]) is False  # an applied step: nothing to take back
    assert f["step"] == 3 and opt.skipped_steps == 0
    assert opt.settle([math.nan, math.nan, 0.0, 0.0]) is True  # a skipped one does not count
    assert f["step"] == 2 and opt.skipped_steps == 1
    assert opt.settle() is False and f["step"] == 2  # no guarded step is open: nothing is fetched, nothing changes
    f["m"].fill_(0.25)
    f["v"].fill_(0.5)
    sd = opt.state_dict()
    assert sd["flat"][0]["skipped"] == 1 and sd["flat"][0]["step"] == 2
    again = _opt()
    again.load_state_dict(sd)
    assert again.skipped_steps == 1 and again._flat[0]["step"] == 2
    assert torch.equal(again._flat[0]["m"], f["m"]) and torch.equal(again._flat[0]["v"], f["v"])
    # a state dict from before the guard has no count
    old = opt.state_dict()
    del old["flat"][0]["skipped"]
    older = _opt()
    older.skipped_steps = 5
    older.load_state_dict(old)
    assert older.skipped_steps == 0 and older._flat[0]["step"] == 2
