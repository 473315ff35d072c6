"""Graph reuse across driftSDE sampling calls (reuse_graph), the host side: the option surface, the state[1] rule that lets a held
step kernel draw a fresh Stepper's Philox counters, the session key, and the cap on held sessions.  No GPU."""
import gc
import weakref

import pytest
import torch
from torch import nn

from instancediff_amd import train_ops
from instancediff_amd.models.SDEs import create_sde
from instancediff_amd.models.SDEs import driftSDE as mod
from instancediff_amd.models.SDEs.driftSDE import driftSDE, session_calls0, session_key, weights_signature


# ---- the option ---------------------------------------------------------------------------------------------------------------------
def test_reuse_graph_is_off_by_default_and_takes_bools_only():
    sde = driftSDE(T=8)
    assert sde.reuse_graph is False and sde.last_session is None
    assert driftSDE(T=8, reuse_graph=None).reuse_graph is False
    assert driftSDE(T=8, reuse_graph=True).reuse_graph is True
    assert driftSDE(T=8, reuse_graph=False).reuse_graph is False
    for bad in (1, 0, "true", "yes", 1.0, [True]):
        with pytest.raises(ValueError):
            driftSDE(T=8, reuse_graph=bad)
        with pytest.raises(ValueError):
            sde.set_reuse_graph(bad)
    assert sde.reuse_graph is False  # a refused value changes nothing


def test_setter_create_sde_and_close_sessions_without_sessions():
    sde = create_sde({}, dict(class_name="driftSDE", T=8, sample_T=4, reuse_graph=True))
    assert sde.reuse_graph is True
    assert create_sde({}, dict(class_name="driftSDE", T=8)).reuse_graph is False
    sde.close_sessions()  # none held: nothing to do
    sde.set_reuse_graph(False)
    assert sde.reuse_graph is False
    sde.set_reuse_graph(True)
    assert sde.reuse_graph is True
    sde.set_reuse_graph(None)
    assert sde.reuse_graph is False


class FakeSession:
    def __init__(self):
        self.closed = 0

    def close(self):
        self.closed += 1


def test_set_reuse_graph_false_closes_the_held_sessions():
    sde = driftSDE(T=8, reuse_graph=True)
    a, b = FakeSession(), FakeSession()
    sde._hold_session("a", a)
    sde._hold_session("b", b)
    sde.set_reuse_graph(True)
    assert (a.closed, b.closed) == (0, 0) and len(sde._sessions) == 2
    sde.set_reuse_graph(False)
    assert (a.closed, b.closed) == (1, 1) and not sde._sessions


def test_at_most_four_sessions_the_least_recently_used_goes_first():
    assert mod.MAX_SESSIONS == 4
    sde = driftSDE(T=8, reuse_graph=True)
    ses = {k: FakeSession() for k in "abcdef"}
    for k in "abcd":
        sde._hold_session(k, ses[k])
    assert list(sde._sessions) == list("abcd") and not any(s.closed for s in ses.values())
    sde._hold_session("a", ses["a"])  # used again: now the most recent
    sde._hold_session("e", ses["e"])
    assert list(sde._sessions) == list("cdae") and ses["b"].closed == 1
    sde._hold_session("f", ses["f"])
    assert list(sde._sessions) == list("daef") and ses["c"].closed == 1
    assert [ses[k].closed for k in "adef"] == [0, 0, 0, 0]
    sde.close_sessions()
    assert not sde._sessions and [ses[k].closed for k in "abcdef"] == [1] * 6


# ---- state[1] -----------------------------------------------------------------------------------------------------------------------
def test_state1_is_the_exact_quotient():
    nper = 256
    assert session_calls0(1000, 1000, nper) == 0
    # the second image of a 4-step chain: x_T draw + 4 steps + x_T draw since the capture
    assert session_calls0(1000 + 6 * nper, 1000, nper, nsteps=4) == 6
    for off0, q in ((0, 1), (17, 12345), (3, (1 << 31) - 5)):
        assert session_calls0(off0 + q * nper, off0, nper, nsteps=4) == q
        # the counters of step i then are those of a fresh Stepper at `off`
        assert off0 + session_calls0(off0 + q * nper, off0, nper) * nper == off0 + q * nper


def test_state1_asks_for_a_recapture():
    nper = 256
    assert session_calls0(1000 + 2 * nper + 2, 1000, nper) is None        # a draw of another size went through the stream
    assert session_calls0(1000 + 2 * nper - 1, 1000, nper) is None
    assert session_calls0(1000 - nper, 1000, nper) is None                # the stream was rewound
    assert session_calls0(0, 1000, nper) is None
    assert session_calls0(nper << 31, 0, nper) is None                    # does not fit the device word
    assert session_calls0(nper * ((1 << 31) - 1), 0, nper) == (1 << 31) - 1
    assert session_calls0(nper * ((1 << 31) - 1), 0, nper, nsteps=1) is None   # nor would the count after the chain's advances
    assert session_calls0(nper * ((1 << 31) - 4), 0, nper, nsteps=4) is None
    assert session_calls0(nper * ((1 << 31) - 5), 0, nper, nsteps=4) == (1 << 31) - 5
    assert session_calls0(5, 5, 0) is None


# ---- the key ------------------------------------------------------------------------------------------------------------------------
class Smm(nn.Module):
    def __init__(self):
        super().__init__()
        self.contexts = nn.Parameter(torch.zeros(2, 3))
        self.register_buffer("tokens", torch.zeros(2, 4, dtype=torch.long))


class Net(nn.Module):
    conv_dtype = "f32"

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(1, 2, 3)
        self.smm = Smm()

    def score_map_modules(self):
        return [self.smm]


class Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(3, 3)


def make(**kw):
    nets = dict(drift_net=Net(), noise_net=Net())
    opts = dict(T=20, max_sigma=0.4, eta=1.0, drift_schedule="sigmoid", noise_schedule="sigmoid", sample_T=4)
    opts.update(kw)
    return driftSDE(nets=nets, **opts), Encoder()


ARGS = dict(kind="plain", rows=1, chw=(1, 32, 32), ctx_shape=(1, 512), sched=(20, 15, 10, 5, 0), order=1, T_stop=0, device="cpu")


def key_of(sde, enc, **kw):
    a = dict(ARGS)
    a.update(kw)
    return session_key(sde, a["kind"], a["rows"], a["chw"], a["ctx_shape"], a["sched"], a["order"], a["T_stop"], enc, a["device"])


def test_key_is_stable_and_hashable():
    sde, enc = make()
    k = key_of(sde, enc)
    assert k == key_of(sde, enc) and hash(k) == hash(key_of(sde, enc))
    assert {k: 1}[key_of(sde, enc)] == 1


@pytest.mark.parametrize("change", [dict(kind="member"), dict(rows=2), dict(chw=(1, 32, 48)), dict(chw=(3, 32, 32)), dict(ctx_shape=(2, 512)),
                                    dict(ctx_shape=None), dict(sched=(20, 10, 0)), dict(sched=None), dict(order=2), dict(T_stop=5),
                                    dict(device="cuda:0")])
def test_key_differs_with_each_argument(change):
    sde, enc = make()
    assert key_of(sde, enc) != key_of(sde, enc, **change)


def test_key_differs_with_the_seed_the_process_and_the_streams():
    sde, enc = make()
    k = key_of(sde, enc)
    sde.set_seed(7)
    assert key_of(sde, enc) != k
    sde.set_seed(0)
    assert key_of(sde, enc) == k
    for attr, val in (("T", 21), ("max_sigma", 0.5), ("eta", 0.5), ("schedule_names", ("cosine", "sigmoid")),
                      ("schedule_names", ("sigmoid", "linear")), ("two_streams", not sde.two_streams)):
        old = getattr(sde, attr)
        setattr(sde, attr, val)
        assert key_of(sde, enc) != k, attr
        setattr(sde, attr, old)
        assert key_of(sde, enc) == k, attr
    assert driftSDE(T=20, drift_schedule="cosine").schedule_names == ("cosine", "sigmoid")


def test_key_differs_with_the_nets_the_encoder_and_their_conv_dtype():
    sde, enc = make()
    k = key_of(sde, enc)
    for which in ("drift_net", "noise_net"):
        old = getattr(sde, which)
        twin = Net()
        twin.load_state_dict(old.state_dict())
        setattr(sde, which, twin)
        assert key_of(sde, enc) != k, which
        setattr(sde, which, old)
        assert key_of(sde, enc) == k
    assert key_of(sde, Encoder()) != k
    sde.noise_net.conv_dtype = "bf16"
    assert key_of(sde, enc) != k
    del sde.noise_net.conv_dtype
    assert key_of(sde, enc) == k


def test_key_follows_the_weights():
    sde, enc = make()
    k = key_of(sde, enc)
    with torch.no_grad():
        sde.drift_net.conv.weight.mul_(1.0001)        # an in-place edit moves _version
    k1 = key_of(sde, enc)
    assert k1 != k and k1[:-1] == k[:-1]              # only the weights signature, the key's last item
    with torch.no_grad():
        sde.noise_net.smm.contexts.add_(1.0)          # a ScoreMapModule's parameter
    k2 = key_of(sde, enc)
    assert k2 != k1
    sde.noise_net.smm.tokens.add_(1)                  # a buffer
    k3 = key_of(sde, enc)
    assert k3 != k2
    with torch.no_grad():
        enc.lin.bias.zero_()                          # the text encoder
    k4 = key_of(sde, enc)
    assert k4 != k3
    sde.drift_net.load_state_dict(sde.noise_net.state_dict())   # a checkpoint load copies in place
    k5 = key_of(sde, enc)
    assert k5 != k4
    sde.drift_net.conv.weight = nn.Parameter(sde.drift_net.conv.weight.detach().clone())   # new storage
    k6 = key_of(sde, enc)
    assert k6 != k5
    train_ops.WEIGHT_EPOCH[0] += 1                    # the fused optimizer writes through raw pointers and bumps this instead
    try:
        assert key_of(sde, enc) != k6
    finally:
        train_ops.WEIGHT_EPOCH[0] -= 1
    assert key_of(sde, enc) == k6


def test_weights_signature_reads_an_ema_wrapper_through_to_its_model():
    class Ema(nn.Module):
        def __init__(self, m):
            super().__init__()
            self.ema_model = m

    sde, enc = make()
    inner = sde.drift_net
    sde.drift_net = Ema(inner)
    k = key_of(sde, enc)
    with torch.no_grad():
        inner.conv.bias.add_(1.0)
    assert key_of(sde, enc) != k
    assert weights_signature([object(), None]) == (train_ops.WEIGHT_EPOCH[0],)   # objects without parameters contribute nothing


def test_cpu_tensors_run_the_per_call_path():
    """capture is off for CPU tensors, so no session can exist: the eligibility check says so before anything is built"""
    sde, _ = make(reuse_graph=True)
    assert sde._session_indices(["a"], torch.zeros(1, 1, 8, 8), None, 4) is None


def test_a_dropped_sde_frees_its_sessions_at_once():
    """The sde owns its sessions; a session and its Stepper reach the sde through a weak proxy.  Without that the three form a cycle
    and the held graphs are destroyed at some later garbage collection, possibly in the middle of another chain's graph capture."""
    sde, _ = make(reuse_graph=True)
    cond = torch.zeros(1, 1, 8, 8)
    ses = driftSDE.Session(sde, "k", 1, cond, None, False)
    ses.stepper = driftSDE.Stepper(ses.sde, ses.x, ses.cond, ses.idx, None, None, timesteps=[20, 15, 10, 5, 0], xa=ses.xa)
    assert ses.stepper.sde.T == 20 and ses.stepper.off_base == 0
    ses.stepper._account(2)  # the Stepper's accounting reaches the sde through the proxy
    assert (sde._calls, sde._off) == (2, 2 * ses.stepper.nper)
    sde._hold_session("k", ses)
    alive = [weakref.ref(sde), weakref.ref(ses), weakref.ref(ses.stepper)]
    gc.disable()
    try:
        del sde, ses
        assert [r() for r in alive] == [None, None, None]
    finally:
        gc.enable()
