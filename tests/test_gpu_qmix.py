"""GPU tests of the QMIX learner against the float64 restatement of ``tests/qmix_helpers.py``: the two persistent GRU kernels,
the fused head, the whole step, centred RMSProp with per-tensor clipping over three trains, and ``QMixModel``.  Bars:
``qmix_helpers.bars()`` (profiles/qmix_parity.md).  Every measured deviation is printed before it is asserted.

Measured on one MI355X (largest over the cases): see profiles/qmix_parity.md."""
import numpy as np
import pytest
import torch

from tests import qmix_helpers as Q

pytestmark = pytest.mark.gpu


def _lib():
    from xingtian_amd import lib as L
    return L, L.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _check(what, got, ref, bar):
    dev = Q.rel(got.cpu().numpy() if torch.is_tensor(got) else got, ref)
    print("{}: {:.3e} (bar {:.3e})".format(what, dev, bar))
    assert dev <= bar, what
    return dev


# ---------------------------------------------------------------------- 1. the persistent GRU kernels
@pytest.mark.parametrize("s,t1,h,ragged", Q.GRU_CASES)
def test_gru_kernels_against_float64(s, t1, h, ragged):
    L, lib = _lib()
    c = Q.gru_case(s, t1, h, ragged)
    st64, out64, hT64, dxg64, dh064 = Q.gru_case_ref(c)
    d = {k: _dev(v) for k, v in c.items()}
    saved, out, hT = _out(t1, s, 4 * h), _out(t1, s, h), _out(s, h)
    L.check(lib.xt_qmix_gru_fwd(L.ptr(d["wg"]), L.ptr(d["wc"]), L.ptr(d["xg"]), L.ptr(d["h0"]), L.ptr(d["lens"]), t1, s, h,
                                L.ptr(saved), L.ptr(out), L.ptr(hT), L.stream_ptr()), "xt_qmix_gru_fwd")
    bar = Q.bars()["gru_fwd"][1]
    _check("saved h", saved[..., 3 * h:], st64, bar)
    _check("out", out, out64, bar)
    _check("final state", hT, hT64, bar)
    assert (out.cpu().numpy()[np.arange(t1)[:, None] >= c["lens"][None, :]] == 0).all()      # exactly zero past the length
    dg3, dh0 = _out(t1, s, 3 * h), _out(s, h)
    L.check(lib.xt_qmix_gru_bwd(L.ptr(d["wg"]), L.ptr(d["wc"]), L.ptr(saved), L.ptr(d["h0"]), L.ptr(d["dout"]), L.ptr(d["dhT"]),
                                L.ptr(d["lens"]), t1, s, h, L.ptr(dg3), L.ptr(dh0), L.stream_ptr()), "xt_qmix_gru_bwd")
    bar = Q.bars()["gru_bwd"][1]
    _check("d(gates)", dg3, dxg64, bar)
    _check("d(h0)", dh0, dh064, bar)


# ---------------------------------------------------------------------- 2. the fused head
@pytest.mark.parametrize("rows,n,a,e,double_q", Q.MIX_CASES)
def test_head_against_float64(rows, n, a, e, double_q):
    L, lib = _lib()
    c = Q.mix_case(rows, n, a, e)
    b, t = c["b"], c["t"]
    loss64, qtot64, y64, dq64, dhyp64 = Q.mix_case_ref(c, n, e, double_q)
    d = {k: _dev(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    qe, qt = _dev(Q.time_major(c["qe"])), _dev(Q.time_major(c["qt"]))
    dq, dhyp, qtot = _out(t + 1, b * n, a), _out(b * t, n * e + 2 * e + 1), _out(b * t, 2)
    rowloss, scal = _out(b * t, dtype=torch.float64), _out(2, dtype=torch.float64)
    L.check(lib.xt_qmix_mix(L.ptr(qe), L.ptr(qt), L.ptr(d["avail"]), L.ptr(d["actions"]), L.ptr(d["hyp_e"]), L.ptr(d["hyp_t"]),
                            L.ptr(d["rewards"]), L.ptr(d["terminated"]), L.ptr(d["mask"]), b, t, n, a, e, 0.99, int(double_q), L.ptr(dq),
                            L.ptr(dhyp), L.ptr(qtot), L.ptr(rowloss), L.ptr(scal[:1]), L.ptr(scal[1:]), L.stream_ptr()), "xt_qmix_mix")
    fwd, bwd = Q.bars()["mix_fwd"][1], Q.bars()["mix_bwd"][1]
    _check("q_tot", qtot[:, 0], qtot64, fwd)
    _check("y (first index of a tie, single available action)", qtot[:, 1], y64, fwd)
    _check("loss", scal[1:], [loss64], fwd)
    assert float(scal[0]) == c["mask"].sum()
    _check("d(q)", dq, Q.time_major(dq64), bwd)
    _check("d(hyp)", dhyp, dhyp64, bwd)
    g = dhyp.cpu().numpy()
    assert g[0, 0] == 0 and g[0, n * e + e] == 0                            # raw zeros have gradient 0
    assert (g[c["mask"].reshape(-1) == 0] == 0).all()                       # rows with mask 0 send nothing back


# ---------------------------------------------------------------------- 3. the whole step, 4. the optimiser
def _net(spec, params, lr=0.0005, clip=10.0):
    from xingtian_amd.model.qmix.qmix_model import HipQmix
    net = HipQmix(spec, seed=0, lr=lr, clip=clip)
    for which in ("eval", "target"):
        net.set_train_weights(params, which)
    return net


@pytest.mark.parametrize("b,n,t", Q.STEP_CASES)
def test_whole_step_against_float64(b, n, t):
    spec, params, case = Q.step_inputs(b, n, t)
    loss64, g64, gap, _ = Q.step_ref(spec, params, case)
    assert gap > 1e-4 and case["mask"].sum() > 0
    net = _net(spec, params)
    loss = float(net.grad_step(*Q.train_args(case)).item())
    bars = Q.bars()
    print("loss {:.3e} (bar {:.3e})".format(abs(loss - loss64) / abs(loss64), bars["step_loss"][1]))
    assert abs(loss - loss64) <= bars["step_loss"][1] * abs(loss64)
    got = net.get_gradients()
    assert list(got) == list(g64) and len(got) == 22
    for k in g64:
        _check(k, got[k], g64[k], bars["step_grad"][1])


def test_three_trains_with_rmsprop_and_target_sync():
    lr, clip = 0.01, 0.5
    spec, params, case = Q.step_inputs(3, 2, 4, reward_scale=4.0)
    net = _net(spec, params, lr, clip)

    def rounds(net):
        out = []
        for i in range(3):
            if i == 2:
                net.sync_target()
            out.append(float(net.grad_step(*Q.train_args(case)).item()))
            net.apply()
        return out, net.params.cpu().numpy().copy()

    losses, flat = rounds(net)
    losses2, flat2 = rounds(_net(spec, params, lr, clip))
    assert losses == losses2 and np.array_equal(flat, flat2)               # bit for bit from one state
    p = {k: v.astype(np.float64) for k, v in params.items()}
    ev = [k for k in p if k.startswith("eval")]
    mg, ms = {k: np.zeros_like(p[k]) for k in ev}, {k: np.ones_like(p[k]) for k in ev}
    above = below = 0
    for i in range(3):
        if i == 2:
            p.update({k.replace("eval", "target", 1): p[k].copy() for k in ev})
        loss64, g64, _, _ = Q.step_ref(spec, p, case)
        norms = Q.rmsprop_ref(p, g64, mg, ms, lr, clip)
        above, below = above + sum(v > clip for v in norms.values()), below + sum(0 < v < clip for v in norms.values())
        assert abs(losses[i] - loss64) <= 1e-4 * abs(loss64), (i, losses[i], loss64)
    assert above and below                                                  # both sides of the per-tensor clip are exercised
    got = net.get_train_weights("eval")
    for k in ev:
        _check(k + " after three trains", got[k], p[k], 1e-5)
    tgt = net.get_train_weights("target")
    for k in ev:      # the target set is the eval set of two trains ago, not today's
        _check(k + " target", tgt[k.replace("eval", "target", 1)], p[k.replace("eval", "target", 1)], 1e-5)
    assert float(net.state[0]) == 3.0


# ---------------------------------------------------------------------- 5. QMixModel
@pytest.mark.parametrize("device", ["gpu", "cpu"])
def test_model_train_and_stepped_inference(device):
    from xingtian_amd.model import model_builder
    spec, params, case = Q.step_inputs(3, 2, 4)
    cfg = dict(n_agents=2, obs_shape=spec.D, rnn_hidden_dim=spec.H, episode_limit=4, n_actions=spec.A, state_shape=spec.sd,
               mixing_embed_dim=spec.E, hypernet_embed=spec.HE, batch_size=3, use_double_q=spec.double_q, SEED=1, DEVICE=device)
    m = model_builder(dict(model_name="QMixModel", scene="train", model_config=cfg))
    loss64, _, _, q64 = Q.step_ref(spec, params, case)
    agent = {k.replace("eval_agent", "explore_agent"): v for k, v in params.items() if k.startswith("eval_agent")}
    if device == "gpu":
        for which in ("eval", "target"):
            m.net.set_train_weights(params, which)
        m.assign_explore_agent()
        got = m.get_weights()
        assert list(got) == list(agent) and all(np.array_equal(got[k], agent[k]) for k in agent)
        loss = m.train(*Q.train_args(case))
        print("train loss {:.3e}".format(abs(loss - loss64) / abs(loss64)))
        assert abs(loss - loss64) <= Q.bars()["step_loss"][1] * abs(loss64)
    else:
        assert m.net.inference_only
        m.set_weights(agent)
    # the explore agent (the weights from before the train), one step at a time, episode 0: the train graph's eval q
    m.reset_hidden_state()
    full = np.flatnonzero(np.asarray(case["lens"][:2]) == spec.T + 1)      # agents of episode 0 whose sequence has the full length
    for t in range(spec.T + 1):
        q = m.infer_actions(case["obs"][:1, t:t + 1])
        assert q.shape == (1, 2, spec.A)
        _check("infer_actions step {}".format(t), q[0, full], q64[0, t, full], 1e-5)
