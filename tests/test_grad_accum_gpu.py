"""Gradient accumulation on the GPU: idiff_gather_segments_acc through the C ABI against torch's fp32 add on the same operands (bit for
bit: one add per element, each owned by one thread), FusedAdam(accum_steps=3) against a plain FusedAdam fed the sum ((g0 + g1) + g2)
with grad_scale 1/3 (bit for bit), then the model's training step, the exchange count and the training driver.

The only tolerances: the guard's norm / coefficient at test_grad_guard_gpu's 1e-5 (reductions under 65 536 terms), the group's mean
loss at 1e-6 (positive fp32 numbers through at most six roundings -- two accumulating adds, the division, three adds over the pyramid's
four records: 6 * 2^-24 = 3.6e-7), and the optional agreement with one big batch at test_configs_gpu's 2e-5."""
import math
import os
import socket

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from instancediff_amd import _lib, pipeline, train_ops as T, trainUM  # noqa: E402
from instancediff_amd.ops import _p, _stream  # noqa: E402
from instancediff_amd.utils.synthetic import make_batch  # noqa: E402

DEV = "cuda"
BADARG = -1  # IDIFF_E_BADARG
K = 3


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# =====================================================================================================
# the kernel
# =====================================================================================================
SEG_LENS = (1, 3, 4095, 4096, None, 4097, 8193)  # None: a record without a source (100 floats of dst it must not touch)
NULL_LEN = 100


def _table():
    """-> (table [nseg, 4] on the device, sources, [(offset, n, src or None)], nblocks, dst length); the offsets are odd (no multiple
    of 4) and leave gaps of 3 / 5 / 7 ... floats between the segments, and a margin behind the last"""
    recs, srcs, rows = [], [], []
    off, blk = 1, 0
    for i, n in enumerate(SEG_LENS):
        src = None if n is None else torch.randn(n, generator=_g(20 + i)).to(DEV)
        n = NULL_LEN if n is None else n
        assert off % 4 != 0
        rows.append((0 if src is None else src.data_ptr(), off, n, blk))
        recs.append((off, n, src))
        srcs.append(src)
        blk += (n + 4095) // 4096
        off += n + 3 + 2 * i
        off += 1 if off % 4 == 0 else 0
    return torch.tensor(rows, dtype=torch.int64).to(DEV), srcs, recs, blk, off + 64


def test_gather_acc_adds_bit_for_bit_and_leaves_the_rest():
    lib = _lib.load()
    tab, srcs, recs, nblocks, total = _table()
    assert nblocks == 1 + 1 + 1 + 1 + 1 + 2 + 3
    before = torch.randn(total, generator=_g(1)).to(DEV)
    want = before.clone()
    for off, n, src in recs:
        assert off + n <= total
        if src is not None:
            want[off:off + n] = before[off:off + n] + src
    outs = []
    for _ in range(2):
        dst = before.clone()
        assert lib.idiff_gather_segments_acc(tab.data_ptr(), len(recs), nblocks, _p(dst), _stream()) == 0
        outs.append(dst)
    torch.cuda.synchronize()
    assert _same_bits(outs[0], want)  # the sums, and every float outside the records with a source: gaps, the NULL range, the margin
    assert _same_bits(outs[0], outs[1])
    off, n, _ = recs[4]
    assert _same_bits(outs[0][off:off + n], before[off:off + n]) and not _same_bits(outs[0], before)
    # the assigning entry point on the same table, for contrast: it zero-fills the NULL range
    dst = before.clone()
    assert lib.idiff_gather_segments(tab.data_ptr(), len(recs), nblocks, _p(dst), _stream()) == 0
    assert float(dst[off:off + n].abs().max()) == 0.0 and _same_bits(dst[recs[5][0]:recs[5][0] + 4097], srcs[5])


def test_gather_acc_refusals_launch_nothing():
    lib = _lib.load()
    tab, _, recs, nblocks, total = _table()
    before = torch.randn(total, generator=_g(2)).to(DEV)
    dst = before.clone()
    launches = lib.idiff_launch_count()
    assert lib.idiff_gather_segments_acc(None, len(recs), nblocks, _p(dst), _stream()) == BADARG
    assert lib.idiff_gather_segments_acc(tab.data_ptr(), len(recs), nblocks, None, _stream()) == BADARG
    for nseg in (0, -1):
        assert lib.idiff_gather_segments_acc(tab.data_ptr(), nseg, nblocks, _p(dst), _stream()) == BADARG
    for nb in (0, -1, 1 << 31):
        assert lib.idiff_gather_segments_acc(tab.data_ptr(), len(recs), nb, _p(dst), _stream()) == BADARG
    torch.cuda.synchronize()
    assert lib.idiff_launch_count() == launches
    assert _same_bits(dst, before)


# =====================================================================================================
# the optimizer on toy parameters
# =====================================================================================================
TOY = (7, 4096, 5000)


def _toy(wd, **kw):
    ps = [nn.Parameter(torch.randn(n, generator=_g(30 + n)).to(DEV)) for n in TOY]
    return T.FusedAdam(ps, lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, **kw), ps


def _toy_grads(group):
    """K micro-gradients per parameter; the first parameter receives none in the middle micro-step of the second group"""
    gs = [[torch.randn(n, generator=_g(1000 * group + 10 * i + j)).to(DEV) for j, n in enumerate(TOY)] for i in range(K)]
    if group == 1:
        gs[1][0] = None
    return gs


def _sum_in_order(gs, j):
    tot = None
    for i in range(K):
        if gs[i][j] is not None:
            tot = gs[i][j].clone() if tot is None else tot + gs[i][j]
    return tot


def _run_toy(wd, **guard):
    acc, pa = _toy(wd, accum_steps=K, **guard)
    ref, pr = _toy(wd, **guard)
    ref.grad_scale = 1.0 / K
    infos = []
    for group in range(2):
        gs = _toy_grads(group)
        epoch0 = T.WEIGHT_EPOCH[0]
        for i in range(K):
            acc.zero_grad()
            for p, g in zip(pa, gs[i]):
                p.grad = g
            assert acc.micro_step == i
            stepped = acc.step()
            assert stepped is (i == K - 1)
            if not stepped:
                assert T.WEIGHT_EPOCH[0] == epoch0 and acc._flat[0]["step"] == group
        sums = [_sum_in_order(gs, j) for j in range(len(TOY))]
        assert _same_bits(acc._flat[0]["g"], torch.cat(sums))  # ((g0 + g1) + g2); (g0 + g2) where the middle one was missing
        ref.zero_grad()
        for p, s in zip(pr, sums):
            p.grad = s
        assert ref.step() is True
        if guard:
            infos.append((acc.last_info.cpu().tolist(), torch.cat(sums).double() / K))
            assert acc.settle() is False and ref.settle() is False
    fa, fr = acc._flat[0], ref._flat[0]
    assert fa["step"] == 2 and fr["step"] == 2
    for key in ("p", "m", "v"):
        assert _same_bits(fa[key], fr[key]), key
    assert not _same_bits(fa["p"], torch.cat([torch.randn(n, generator=_g(30 + n)) for n in TOY]).to(DEV))  # and something happened
    return infos


@pytest.mark.parametrize("wd", [pytest.param(0.0, id="no-wd"), pytest.param(1e-2, id="wd")])
def test_fused_adam_accumulates_then_steps_on_the_mean(wd):
    _run_toy(wd)


@pytest.mark.parametrize("wd", [pytest.param(0.0, id="no-wd"), pytest.param(1e-2, id="wd")])
def test_fused_adam_clips_the_mean_gradient(wd):
    c = 1.0  # the mean of three N(0, 1) gradients over 9103 elements has a norm near sqrt(9103 / 3) = 55: the clip is active
    for info, mean in _run_toy(wd, max_grad_norm=c):
        norm = float(mean.norm())
        coef = min(1.0, c / (norm + 1e-6))
        print(f"wd {wd}: norm {info[0]!r} vs fp64 {norm!r}, coef {info[1]!r} vs {coef!r}")
        assert coef < 0.1
        assert abs(info[0] - norm) <= 1e-5 * norm and abs(info[1] - coef) <= 1e-5 * coef
        assert info[2:] == [1.0, 0.0]


# =====================================================================================================
# the model's training step (32 x 32, micro-batch 2, k = 3, T = 20, injected t and eps)
# =====================================================================================================
def _model(**kw):
    model, sde = pipeline.build(phase="train", device=torch.device(DEV), T=20, seed=0, score_map_dropout=0.0, **kw)
    model.set_train()
    return model, sde


def _feed(model, sde, item):
    batch, t, eps = item
    model.input = batch['input'].to(DEV)
    model.target = batch['target'].to(DEV).clone()
    model.names = list(batch['names'])
    model.A_emb = batch['A_emb'].to(DEV)
    model.t, model.drift_noised_x, _, model.std_noise, _ = sde.forward_diffusion(model.target, model.input, t=t, eps=eps.to(DEV))
    model.std_noise = model.std_noise.clone()


def _opts(model):
    return (("drift", model.drift_optimizer), ("noise", model.noise_optimizer))


def _opt_state(model):
    return [o._flat[0][k].clone() for _, o in _opts(model) for k in ("p", "m", "v")]


def _loss_of(rec):
    r = rec.double().cpu()
    return dict(dl=float(r[0]), nl=float(r[1]), dsml=float(r[2:6].sum()) / 2.0, nsml=float(r[6:10].sum()) / 2.0)


@pytest.fixture(scope="module")
def micro():
    """three micro-batches of 2 and, with the option off, the gradient and the loss record of each on the initial weights (no step
    is taken) -> dict(items, grads={'drift' / 'noise': [g0, g1, g2]}, recs, model, sde); nobody writes to the tensors or steps the model"""
    ts = ([5, 17], [2, 11], [20, 8])
    items = []
    for i, tt in enumerate(ts):
        batch = make_batch(2, 32, seed=3 + i)
        eps = torch.randn(batch['input'].shape, generator=_g(7 + i))
        items.append((batch, torch.tensor(tt).reshape(2, 1, 1, 1), eps))
    model, sde = _model()
    grads, recs = {"drift": [], "noise": []}, []
    for item in items:
        _feed(model, sde, item)
        rec, _, _, _ = T.forward_backward_inputRes(model)
        recs.append(rec.clone())
        for key, o in _opts(model):
            grads[key].append(o.flat_grads()[0].clone())
    return dict(items=items, grads=grads, recs=recs, model=model, sde=sde)


def test_model_accumulates_three_micro_batches_and_steps_once(micro):
    lib = _lib.load()
    model, sde = _model(accum_steps=K)
    assert model.accum_steps == K and model.stepped is False
    before, epoch0 = _opt_state(model), T.WEIGHT_EPOCH[0]
    for a, b in zip(before, _opt_state(micro["model"])):
        assert _same_bits(a, b)  # both models start from the same weights
    seen = {}
    for key, o in _opts(model):  # the flat gradient and the scale the group's end hands to Adam
        def spy(scale, o=o, key=key, inner=o._apply):
            seen[key] = (o._flat[0]["g"].clone(), scale)
            return inner(scale)
        o._apply = spy
    for i in range(2):
        _feed(model, sde, micro["items"][i])
        loss, _ = model.optimize_parameters()
        assert loss is None and model.stepped is False
    for a, b in zip(before, _opt_state(model)):
        assert _same_bits(a, b)
    assert T.WEIGHT_EPOCH[0] == epoch0 and not seen and model.loss_info["num"] == 0
    for _, o in _opts(model):
        assert o.micro_step == 2 and o.boundary_next and o._flat[0]["step"] == 0
    _feed(model, sde, micro["items"][2])
    launches = lib.idiff_launch_count()
    loss, _ = model.optimize_parameters()
    assert model.stepped is True and T.WEIGHT_EPOCH[0] > epoch0
    sums = {}
    for key, o in _opts(model):
        g0, g1, g2 = micro["grads"][key]
        sums[key] = (g0 + g1) + g2
        flat, scale = seen[key]
        assert _same_bits(flat, sums[key]), key
        assert scale == 1.0 / K and o.micro_step == 0 and o._flat[0]["step"] == 1
    # the step itself: a model with the option off, handed the same sum and 1/3 as its grad_scale, lands on the same bits
    ref, _ = _model()
    for key, o in _opts(ref):
        o.flat_grads()[0].copy_(sums[key])
        o.grad_scale = 1.0 / K
        assert o.step() is True
    for a, b in zip(_opt_state(model), _opt_state(ref)):
        assert _same_bits(a, b)
    assert not _same_bits(before[0], _opt_state(model)[0])
    # the losses: the mean of the three records, once
    li = model.loss_info
    assert li["num"] == 1 and loss == li["latest"]["l"]
    parts = [_loss_of(r) for r in micro["recs"]]
    for k in ("dl", "nl", "dsml", "nsml"):
        want = sum(p[k] for p in parts) / K
        print(f"{k}: group mean {li['latest'][k]!r} vs fp64 mean of the three records {want!r}")
        assert want > 0 and abs(li["latest"][k] - want) <= 1e-6 * want, k
    want = sum(sum(p.values()) for p in parts) / K
    assert abs(loss - want) <= 1e-6 * want
    for ema in (model.dp_ema, model.np_ema):
        assert int(ema.step) == 1  # once per optimizer step, not per micro-step
    print(f"library launches of the boundary micro-step: {lib.idiff_launch_count() - launches}")


def test_accumulated_mean_agrees_with_one_batch_of_six(micro):
    """the accumulated flat gradient / 3 against the flat gradient of the three micro-batches fed as ONE batch of 6, relative to the
    largest magnitude; the bound is test_configs_gpu's for the same quantity (2e-5 at 256 x 256, batch 32)"""
    model, sde = micro["model"], micro["sde"]
    items = micro["items"]
    batch = {k: (torch.cat([it[0][k] for it in items]) if torch.is_tensor(items[0][0][k]) else sum((list(it[0][k]) for it in items), []))
             for k in items[0][0]}
    _feed(model, sde, (batch, torch.cat([it[1] for it in items]), torch.cat([it[2] for it in items])))
    T.forward_backward_inputRes(model)
    for key, o in _opts(model):
        full = o.flat_grads()[0].double()
        g0, g1, g2 = micro["grads"][key]
        mean = ((g0 + g1) + g2).double() / K
        err = float((full - mean).abs().max() / full.abs().max())
        print(f"{key}: accumulated mean of 3 x 2 vs one batch of 6 at 32 x 32: rel err {err:.2e} (bound 2e-5)")
        assert err < 2e-5, (key, err)


def test_accum_steps_one_is_todays_step(micro):
    lib = _lib.load()
    plain, sde_a = _model()
    one, sde_b = _model(accum_steps=1)
    counts = []
    for it in range(2):
        for model, sde in ((plain, sde_a), (one, sde_b)):
            _feed(model, sde, micro["items"][it])
            n0 = lib.idiff_launch_count()
            loss, _ = model.optimize_parameters()
            counts.append((lib.idiff_launch_count() - n0, loss))
            assert model.stepped is True
    assert counts[0] == counts[1] and counts[2] == counts[3]  # the same launches, the same loss
    for a, b in zip(_opt_state(plain), _opt_state(one)):
        assert _same_bits(a, b)
    assert one.drift_optimizer._flat[0]["step"] == 2 and one.loss_info["num"] == 2


def test_nan_in_one_micro_batch_skips_the_group_once(micro):
    model, sde = _model(accum_steps=K, skip_nonfinite_steps=True)
    before = _opt_state(model)
    for i in range(K):
        _feed(model, sde, micro["items"][i])
        if i == 1:
            model.target[0, 0, 3, 4] = math.nan      # the drift net's loss target is input - target ...
            model.std_noise[1, 0, 7, 1] = math.nan   # ... and the noise net's is std_noise
        model.optimize_parameters()
        assert model.stepped is (i == K - 1)
        assert model.skipped_steps == (1 if i == K - 1 else 0)
    for a, b in zip(before, _opt_state(model)):
        assert _same_bits(a, b)
    gi = model.grad_info
    assert gi["skipped_steps"] == 1 and gi["drift"]["skipped"] is True and gi["noise"]["skipped"] is True
    for _, o in _opts(model):
        assert o._flat[0]["step"] == 0 and o.skipped_steps == 1 and o.micro_step == 0
    for i in range(K):  # a clean group: its first micro-step overwrites the NaNs in the flat buffers
        _feed(model, sde, micro["items"][i])
        loss, _ = model.optimize_parameters()
    assert model.stepped is True and math.isfinite(loss)
    after = _opt_state(model)
    assert all(bool(torch.isfinite(x).all()) for x in after)
    assert not _same_bits(before[0], after[0]) and not _same_bits(before[3], after[3])
    assert model.skipped_steps == 1 and model.grad_info["drift"]["skipped"] is False
    for _, o in _opts(model):
        assert o._flat[0]["step"] == 1 and o.skipped_steps == 1


# =====================================================================================================
# the exchange (RCCL at world size 1) and the driver
# =====================================================================================================
@pytest.fixture()
def rccl_world1():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


def test_exchange_runs_once_per_optimizer_step(micro, rccl_world1):
    from instancediff_amd.parallel import GradSync
    plain, sde_a = _model(accum_steps=2)
    synced, sde_b = pipeline.build(phase="train", device=torch.device(DEV), T=20, seed=0, dist=True, score_map_dropout=0.0, accum_steps=2)
    synced.set_train()
    assert synced.grad_sync is not None
    gs = synced.grad_sync = GradSync(single_rank_collectives=True)
    assert gs.active
    calls = []  # (micro-step, what)
    step = [0]
    start, finish = gs.start, gs.finish
    gs.start = lambda flats: (calls.append((step[0], "start")), start(flats))[1]
    gs.finish = lambda: (calls.append((step[0], "finish")), finish())[1]
    for i in range(4):
        step[0] = i
        for model, sde in ((plain, sde_a), (synced, sde_b)):
            _feed(model, sde, micro["items"][i % 3])
            model.optimize_parameters()
            assert model.stepped is (i % 2 == 1)
        assert not gs._pending
    assert calls == [(1, "start"), (1, "start"), (1, "finish"), (3, "start"), (3, "start"), (3, "finish")]  # one per optimizer, per step
    for a, b in zip(_opt_state(plain), _opt_state(synced)):
        assert _same_bits(a, b)
    assert synced.drift_optimizer._flat[0]["step"] == 2


def test_train_driver_counts_optimizer_steps(tmp_path, monkeypatch, capsys):
    txt = open(pipeline.DEFAULT_YAML).read()
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_accum").replace("image_size: 64", "image_size: 32")
    txt = txt.replace("T: 100", "T: 4").replace("val_freq: 3", "val_freq: 1000\n  max_iters: 2").replace("save_checkpoint_freq: 8", "save_checkpoint_freq: 2")
    txt = txt.replace("path:\n", f"path:\n  root: {tmp_path}\n")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    fed = []
    inner = trainUM.iterate_batches

    def counting(dataset, bs, **kw):
        for td in inner(dataset, bs, **kw):
            if kw.get("shuffle"):  # the training loader (validation iterates without)
                fed.append(len(td["name"]))
            yield td
    monkeypatch.setattr(trainUM, "iterate_batches", counting)
    steps = trainUM.main(["-opt", str(cfg), "--accum-steps", "2"])
    assert steps == 2 and fed == [4, 4, 4, 4]
    out = capsys.readouterr().out
    assert "effective batch: 8 (batch_size 4 x accum_steps 2 x world 1)" in out and "Discarded" not in out
    found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs]
    assert any(f.endswith("2_DN.pth") for f in found) and any(f.endswith("latest_NN.pth") for f in found)
    states = [f for f in found if f.endswith("2.state")]
    assert len(states) == 1
    opt = pipeline.load_options(str(cfg), is_train=True)
    model, _ = pipeline.build(opt=opt, phase="train", device=torch.device(DEV), T=4, accum_steps=2)
    state = model.load_training_state(states[0])
    assert state["iter"] == 2
    model.resume_training(state)
    for _, o in _opts(model):
        assert o._flat[0]["step"] == 2 and o.micro_step == 0 and float(o._flat[0]["v"].abs().max()) > 0


def test_epoch_checkpoint_waits_for_the_open_group(tmp_path, monkeypatch, capsys):
    """8 images in loader batches of 4, k = 3: epoch 0 ends with two micro-gradients held, so its checkpoint (epochs 0, 5, ...) is
    written when the first batch of epoch 1 closes the group -- as epoch 0, at optimizer step 1"""
    txt = open(pipeline.DEFAULT_YAML).read()
    txt = txt.replace("name: UM_IDDM_SM_IB", "name: drv_accum3").replace("image_size: 64", "image_size: 32")
    txt = txt.replace("T: 100", "T: 4").replace("val_freq: 3", "val_freq: 1000\n  max_iters: 1").replace("save_checkpoint_freq: 8", "save_checkpoint_freq: 1000")
    txt = txt.replace("path:\n", f"path:\n  root: {tmp_path}\n")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(txt)
    fed = []
    inner = trainUM.iterate_batches

    def counting(dataset, bs, **kw):
        for td in inner(dataset, bs, **kw):
            fed.append(kw.get("seed"))  # the epoch
            yield td
    monkeypatch.setattr(trainUM, "iterate_batches", counting)
    assert trainUM.main(["-opt", str(cfg), "--accum-steps", "3"]) == 1
    assert fed == [0, 0, 1]
    out = capsys.readouterr().out
    assert "effective batch: 12 " in out and "Discarded" not in out
    found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs]
    assert any(f.endswith("epoch_0_DN.pth") for f in found)
    states = [f for f in found if f.endswith(".state")]
    assert [os.path.basename(f) for f in states] == ["1.state"]
    state = torch.load(states[0], map_location="cpu", weights_only=True)
    assert state["epoch"] == 0 and state["iter"] == 1 and state["optimizers"][0]["flat"][0]["step"] == 1
