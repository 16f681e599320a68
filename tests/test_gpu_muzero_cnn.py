"""GPU tests of the fused dynamics unroll (``xt_mz_set_dyn_fused``) and of the ``MuzeroCnn`` learner (``xt_mz_create_conv``)
against the float64 restatement of ``tests/muzero_helpers.py`` at its standing bars: loss 1e-4, every gradient tensor 1e-5.
Every measured deviation is printed before it is asserted (profiles/muzero_cnn_parity.md)."""
import numpy as np
import pytest

from tests import muzero_helpers as MH
from tests.dqn_helpers import rel_max

pytestmark = pytest.mark.gpu

PONG = dict(value_range=(-21, 21), reward_range=(-2, 2))


def _step(spec, w, batch, fused, obs_type="float32", max_batch=None, sentinel=None):
    """one grad_step of a fresh net -> (net, loss, gradients)"""
    from xingtian_amd.model.muzero.muzero_model import HipMuzero, obs_as_device_input
    net = HipMuzero(spec, max_batch=max_batch or len(batch[0]), seed=1, dyn_fused=fused)
    net.set_weights(w)
    if sentinel is not None:
        net.workspace.fill_(sentinel)
    loss = float(net.grad_step(obs_as_device_input(spec, batch[0], obs_type), *batch[1:]).item())
    return net, loss, net.get_gradients()


def _check(tag, loss, grads, loss_ref, grads_ref):
    errs = MH.grad_errors(grads, grads_ref)
    worst = max(errs.items(), key=lambda kv: kv[1][0] if kv[1][1] == "rel" else 0.0)
    eloss = abs(loss - loss_ref) / abs(loss_ref)
    print("mz {}: loss {:.3e}, worst gradient {} {:.3e}".format(tag, eloss, worst[0], worst[1][0]))
    assert np.isfinite(loss) and eloss <= MH.BAR_LOSS, (tag, loss, loss_ref)
    for k, (e, kind) in errs.items():
        assert e <= (MH.BAR_GRAD if kind == "rel" else 1e-12), (tag, k, e, kind)


# (hidden, trunk width): one column tile; fewer tiles than the 8 wavefronts; 10 tiles, no multiple of 8; the cap
WIDTHS = [(16, 16), (48, 64), (16, 160), (256, 256)]


@pytest.mark.parametrize("unroll", [1, 2, 5])
@pytest.mark.parametrize("b_of", [lambda r: 1, lambda r: r - 1, lambda r: r, lambda r: r + 1, lambda r: 2 * r + 3], ids=["1", "R-1", "R", "R+1", "2R+3"])
@pytest.mark.parametrize("rows", [16, 32])
@pytest.mark.parametrize("hidden,trunk", WIDTHS)
def test_fused_unroll_against_float64(hidden, trunk, rows, b_of, unroll):
    from xingtian_amd.model.muzero.muzero_model import mlp_spec
    b, seed = b_of(rows), hidden + trunk + unroll
    spec = mlp_spec((8,), 3, trunk, hidden, unroll, **PONG)
    w, batch = MH.seeded_weights(spec, seed), MH.make_batch(spec, b, seed + 1)
    loss_ref, grads_ref = MH.Twin(spec, w).loss_and_grads(batch[0].astype(np.float64), *batch[1:])
    for fused in (0, rows):      # the per-layer chain of the same build meets the bars too: a miss is the fused kernels'
        _, loss, grads = _step(spec, w, batch, fused)
        _check("H{} N{} R{} B{} U{} fused {}".format(hidden, trunk, rows, b, unroll, fused), loss, grads, loss_ref, grads_ref)


def test_fused_unroll_is_deterministic_and_leaves_rows_past_b_alone():
    from xingtian_amd.model.muzero.muzero_model import mlp_spec
    spec = mlp_spec((8,), 3, 160, 48, 5, **PONG)
    w, batch = MH.seeded_weights(spec, 7), MH.make_batch(spec, 19, 8)
    sentinel = -6.5e30
    nets = [_step(spec, w, batch, fused, max_batch=40, sentinel=sentinel)[0] for fused in (32, 32, 0)]
    g = [n.grads.cpu().numpy().view(np.uint32) for n in nets]
    assert np.array_equal(g[0], g[1])                            # run to run, bit for bit
    untouched = [(n.workspace == sentinel).cpu().numpy() for n in nets]
    assert untouched[2].any() and np.array_equal(untouched[0], untouched[2])      # it writes where the per-layer chain writes


# ---------------------------------------------------------------------- the MuzeroCnn learner
def _cnn_case(state, a, hidden_out, unroll, b, obs_type, fused, seed):
    from xingtian_amd.model.muzero.muzero_model import cnn_spec, obs_as_device_input
    spec = cnn_spec(state, a, hidden_out, unroll, obs_type=obs_type, **PONG)
    w, batch = MH.seeded_weights(spec, seed), MH.make_batch(spec, b, seed + 1, obs_type)
    x64 = MH.network_input(spec, batch[0], obs_type)
    twin = MH.Twin(spec, w)
    loss_ref, grads_ref = twin.loss_and_grads(x64, *batch[1:])
    tag = "cnn {} H{} {} B{} U{} fused {}".format(state[0], hidden_out, obs_type, b, unroll, fused)
    net, loss, grads = _step(spec, w, batch, fused, obs_type)
    _check(tag, loss, grads, loss_ref, grads_ref)
    x = obs_as_device_input(spec, batch[0], obs_type)
    got = net.initial(x)
    for g, r in zip(got, twin.initial(x64)):
        assert rel_max(g, r) <= MH.BAR_LOSS, tag
    acts = np.arange(b) % a
    for g, r in zip(net.recurrent(got[2], acts), twin.recurrent(got[2], acts)):
        assert rel_max(g, r) <= MH.BAR_LOSS, tag
    # one train: the loss again, and TF Adam's first step from the gradient the device holds (held to float64 above)
    assert net.train_step(x, *batch[1:]) == loss
    g_dev, after = net.get_gradients(), net.get_weights()
    for k, v in w.items():
        want = MH.adam_tf(v.astype(np.float64), g_dev[k].astype(np.float64), 0.0, 0.0, 1)[0]
        assert rel_max(after[k], want) <= MH.BAR_ADAM, (tag, k)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("unroll", [1, 5])
@pytest.mark.parametrize("b", [3, 33])
@pytest.mark.parametrize("obs_type", ["uint8", "float32", "int8"])
@pytest.mark.parametrize("hidden_out", [16, 256])
def test_cnn_learner_against_float64(hidden_out, obs_type, b, unroll, fused):
    _cnn_case((36, 36, 4), 3, hidden_out, unroll, b, obs_type, fused, 3 + b + unroll)


def test_cnn_learner_at_the_example_frame_size():
    _cnn_case((84, 84, 4), 4, 256, 5, 8, "uint8", 1, 5)


def test_model_builder_opts_a_cnn_learner_in():
    from xingtian_amd.model import model_builder
    cfg = dict(reward_min=-2, reward_max=2, value_min=-21, value_max=21, obs_type="uint8", DEVICE="gpu", SEED=2, td_step=2)
    info = dict(model_name="MuzeroCnn", state_dim=[36, 36, 4], action_dim=3, type="learner", model_config=cfg)
    with pytest.raises(NotImplementedError, match="Dense representation chains.*DEVICE_UPDATE"):
        model_builder(info)
    model = model_builder(dict(info, model_config=dict(cfg, DEVICE_UPDATE=True)))
    assert model.net.conv and model.net.dyn_fused == 1
    obs, actions, tv, tr, tp = MH.make_batch(model.spec, 8, 4, "uint8")
    before = model.get_weights()
    loss = model.train([obs, actions, np.ones((8, 1))], [tv, tr, tp])
    assert np.isfinite(loss) and all(not np.array_equal(v, before[k]) for k, v in model.get_weights().items())
    with pytest.raises(TypeError, match="uint8"):
        model.net.grad_step(obs.astype(np.float32), actions, tv, tr, tp)
