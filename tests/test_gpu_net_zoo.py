"""The whole update step on every configurable network shape (tests/net_zoo_helpers.py) against the float64 oracle.

Per row, on a net whose gradient buffer and workspace start as NaN: (1) the plan the library reports for the step
(``xt_net_last_step_report``) is the row's, and every workspace capacity is respected; (2) loss, every gradient tensor, the
gradient norm and the post-step parameters agree with the reference of the row's entry point, at the bars of that entry
point's existing whole-step test (``net_zoo_helpers.BARS``); (3) a second step from the restored parameters, on the
workspace the first one left behind, is the first bit for bit.  Measured figures: profiles/net_zoo_parity.md."""
import json
import time

import numpy as np
import pytest
import torch

import net_zoo_helpers as Z
from test_gpu_learner import assert_update_close

pytestmark = pytest.mark.gpu

# floats at the end of the workspace that xt_net_bind zeroes and the kernels re-arm themselves (ticket counters of the
# gradient reduction, the two hand-over blocks of the folded IO tail): everything in front of them is scratch that a step
# must write before it reads
WS_ARMED_TAIL = 32 * 66 + 8 + 4


def _up(a, dt=None):
    a = np.ascontiguousarray(a if dt is None else np.asarray(a, dt))
    return torch.from_numpy(a).cuda()


def _run(row, net, target, dev):
    """one step through the row's entry point -> (loss, lr) ; the gradient stays in net.grads"""
    entry, i = row["entry"], dev
    if entry == "ppo_step":
        c = net.make_ppo_cfg(dict(Z.PPO_CFG, BATCH_SIZE=Z.frames(row)))
        lo = net.ppo_step(c, i["obs"], i["idx"], i["action"], i["logp"], i["adv"], i["old_v"], i["target_v"], apply=True)
    elif entry == "impala_step":
        c = net.make_impala_cfg(Z.IMPALA_LR, Z.IMPALA_CLIP, row["batch"][0])
        lo = net.impala_step(c, i["obs"], i["bp"], i["action"], i["done"], i["reward"], apply=True)
    elif entry == "keras_impala_step":
        lo = net.keras_impala_step(i["obs"], i["idx"], i["adv"], i["onehot"], i["target_v"], Z.KERAS_ENT)
        lo = lo.clone()
        net.adam_keras(Z.KERAS_LR, 0)
    else:
        lo = net.dqn_step(target, i["cur"], i["nxt"], i["slots"], i["action"], i["reward"], i["done"], Z.DQN_GAMMA,
                          row["args"]["dueling"], False)
    torch.cuda.synchronize()
    return float(lo.cpu().numpy()[0])


def _device_inputs(row, net, inp):
    e = row["entry"]
    if e == "ppo_step":
        gauss = row["args"]["action_type"] == Z.G
        return dict(obs=net.to_device_obs(inp["obs"]), idx=_up(inp["idx"]),
                    action=_up(inp["action"], np.float32 if gauss else np.int32), logp=_up(inp["logp"].reshape(-1), np.float32),
                    adv=_up(inp["adv"].reshape(-1), np.float64), old_v=_up(inp["old_v"].reshape(-1), np.float32),
                    target_v=_up(inp["target_v"].reshape(-1), np.float64))
    if e == "impala_step":
        return dict(obs=net.to_device_obs(inp["obs"]), bp=_up(inp["bp"]), action=_up(inp["action"]),
                    done=_up(inp["done"].astype(np.uint8)), reward=_up(inp["reward"]))
    if e == "keras_impala_step":
        return dict(obs=net.to_device_obs(inp["obs"]), idx=_up(inp["idx"]), adv=_up(inp["adv"].reshape(-1), np.float32),
                    onehot=_up(inp["onehot"], np.float32), target_v=_up(inp["target_v"].reshape(-1), np.float32))
    return dict(cur=net.to_device_obs(inp["cur"]), nxt=net.to_device_obs(inp["nxt"]), slots=_up(inp["slots"]),
                action=_up(inp["action"]), reward=_up(inp["reward"], np.float64), done=_up(inp["done"], np.uint8))


def _check_capacities(rep, spec, b):
    last = rep["layers"] - 1
    for li, (l, lay) in enumerate(zip(rep["layer"], spec.layers)):
        m = b * lay.OH * lay.OW
        assert l["ksplit"] >= 1 and l["ksplit"] * m * lay.N <= rep["partial_floats"], (li, l)
        assert 1 <= l["msplit"] <= l["slab_cap"], (li, l)
        assert l["deferred"] == int(l["deferred"] and l["ksplit"] > 1), (li, l)
        if l["npre"]:      # pre-reduced squared-norm partials belong to the net's last layer, written final by one slab
            assert li == last and l["msplit"] == 1 and li > min(i for i, x in enumerate(rep["layer"]) if x["trunk"] == l["trunk"])
        assert l["preact"] == int(lay.act in Z.PREACT), (li, l)
    assert 0 < rep["finish_blocks"] <= rep["max_norm_partials"]
    assert rep["head_chunks"] == (b + 7) // 8
    if Z.head_class(rep["head_path"]) in ("ppo_fused", "gauss_fused"):      # (the IMPALA word is the v-trace kernel's: no such bit)
        ends = [max(i for i, x in enumerate(rep["layer"]) if x["trunk"] == tr) for tr in range(rep["trunks"])]
        assert (rep["head_path"] >> 8) & 1 == rep["layer"][ends[0]]["deferred"]      # XT_HEAD_PART_SHIFT: the head summed the partials


@pytest.mark.parametrize("rid", Z.ROW_IDS)
def test_whole_step_on_every_network_shape(rid):
    from xingtian_amd import lib as L
    from xingtian_amd.model.hip_net import HipActorCritic
    t0 = time.perf_counter()
    row = Z.ROWS[Z.ROW_IDS.index(rid)]
    ref = Z.reference(row)
    spec, ospec, out, b = ref["spec"], ref["ospec"], ref["out"], Z.frames(row)
    old = L.set_tuning(**row["tuning"]) if row["tuning"] else {}
    try:
        net = HipActorCritic(spec, max_batch=b, seed=0)
        target = None
        if row["entry"] == "dqn_step":
            target = HipActorCritic(spec, max_batch=b, seed=0)
            net.set_weights(Z.DH.to_keras_names(spec, ospec, ref["params"]))
            target.set_weights(Z.DH.to_keras_names(spec, ospec, ref["target_params"]))
            names = Z.DH.name_map(spec, ospec)
        else:
            net.set_weights({k: v.reshape(spec.names[k][1]) for k, v in ref["params"].items()})
            names = {k: k for k in ref["params"]}
        if row["gauss_fused"]:
            net.set_gauss_fused(True)
        dev = _device_inputs(row, net, ref["inputs"])
        net.grads.fill_(float("nan"))
        net.workspace[:net.workspace.numel() - WS_ARMED_TAIL].fill_(float("nan"))
        torch.cuda.synchronize()
        saved = [x.clone() for x in (net.params, net.adam_m, net.adam_v, net.adam_state)]
        w_init = net.get_weights()

        loss = _run(row, net, target, dev)
        rep = net.last_step_report()
        grads, weights, flat_g, flat_p = net.grads_dict(), net.get_weights(), net.grads.clone(), net.params.clone()
        state = net.adam_state.cpu().numpy()

        # (3) the same step again from the restored parameters, on the workspace the first one left
        for dst, src in zip((net.params, net.adam_m, net.adam_v, net.adam_state), saved):
            dst.copy_(src)
        net.touch()
        loss2 = _run(row, net, target, dev)
        rep2 = net.last_step_report()
    finally:
        if old:
            L.set_tuning(**old)

    # (1) the plan
    facts = Z.report_facts(rep, spec)
    want = dict(row["expect"], pad=None, dense_conv=None)

    # (2) parity with the float64 reference, the bars of the entry point's existing whole-step test
    loss_e = abs(loss - float(out["loss"])) / max(1.0, abs(float(out["loss"])))
    worst, worst_k = 0.0, None
    for h, o in names.items():
        r = out["grads"][o]
        g = grads[h].reshape(r.shape)
        assert np.isfinite(g).all(), (rid, h, "an element of the gradient was never written")
        if not np.any(r):
            assert not np.any(g), (rid, h)
            continue
        e = Z.rel_err(g, r)
        if e > worst:
            worst, worst_k = e, h
    gn_e = None
    if out["gnorm"] is not None:
        gn_e = abs(float(state[4]) - float(out["gnorm"])) / float(out["gnorm"])
    upd_e = None
    if out["params"] is not None:
        upd_e = 0.0
        for k, r in out["params"].items():
            init = np.asarray(ref["params"][k], np.float64).reshape(r.shape)
            full = np.abs(r - init) >= 0.5 * out["lr"]
            if full.any():
                d = (np.asarray(weights[k], np.float64).reshape(r.shape) - r)[full]
                upd_e = max(upd_e, float(np.linalg.norm(d) / np.linalg.norm((r - init)[full])))
    lay = rep["layer"]
    print("ZOO " + json.dumps(dict(
        id=rid, head=facts["head"], ksplit=[l["ksplit"] for l in lay], deferred=[l["deferred"] for l in lay],
        msplit=[l["msplit"] for l in lay], slab_cap=[l["slab_cap"] for l in lay], mask=[l["mask_valid"] for l in lay],
        npre=[l["npre"] for l in lay], fuse12=rep["fwd_fuse12"], fuse21=rep["bwd_fuse21"], tail=rep["tail_overlap"],
        form=rep["finish_form"], blocks=rep["finish_blocks"], loss=loss_e, grad=worst, grad_k=worst_k, gnorm=gn_e,
        update=upd_e, seconds=round(time.perf_counter() - t0, 2))))
    assert facts == want, (rid, {k: (want[k], facts[k]) for k in want if want[k] != facts[k]})
    _check_capacities(rep, spec, b)
    assert loss_e <= Z.BARS["loss"], (rid, loss, float(out["loss"]))
    assert worst < Z.BARS["grad"], (rid, worst_k, worst)
    if gn_e is not None:
        assert gn_e < Z.BARS["gnorm"], (rid, float(state[4]), float(out["gnorm"]))
    if out["params"] is not None:
        got = {k: weights[k] for k in out["params"]}
        assert_update_close(got, out["params"], {k: w_init[k] for k in out["params"]}, out["lr"], rid)

    # (3) bit for bit
    assert loss2 == loss and rep2 == rep, (rid, loss, loss2)
    assert torch.equal(torch.nan_to_num(net.grads, nan=0.0), torch.nan_to_num(flat_g, nan=0.0)), rid
    assert torch.equal(torch.nan_to_num(net.params, nan=0.0), torch.nan_to_num(flat_p, nan=0.0)), rid
    g2, w2 = net.grads_dict(), net.get_weights()
    assert all(np.array_equal(g2[k], grads[k]) for k in grads) and all(np.array_equal(w2[k], weights[k]) for k in weights), rid
