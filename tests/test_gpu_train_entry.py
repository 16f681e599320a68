"""The two whole-update entry points as the learners call them: ``xt_net_ppo_train`` / ``xt_net_impala_train`` on the
case tables of tests/train_entry_helpers.py.

a. the minibatch / chunk loop against the same library stepped by the test, bit for bit;
b. the loop against the float64 oracle, at the bars of tests/test_gpu_learner.py's train tests;
c. a replayed hipGraph against the eager call after every change of a cfg field, a pointer, ``n`` or a net switch;
d. one graph, the same pointers, new contents;
e. the eight-slot cache: eviction of the least recently used graph;
f. eager and graph calls interleaved, and a rebind;
g. refusals, one of them inside a capture, leave the net usable.

Tensors only; every run starts from the same saved parameters and a reset optimiser.  ``-s`` prints the measured figures
(profiles/train_entry_parity.md).
"""
import ctypes

import numpy as np
import pytest
import torch

import train_entry_helpers as H
from oracle import nets

pytestmark = pytest.mark.gpu


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _at(t, elems):
    """device address of element ``elems`` of a tensor"""
    return ctypes.c_void_p(t.data_ptr() + int(elems) * t.element_size())


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_state(got, want, tag):
    assert sorted(got) == sorted(want), tag
    for k in want:
        assert same(got[k], want[k]), (tag, k, got[k].ravel()[:4], want[k].ravel()[:4])


# ------------------------------------------------------------------------------------------------ one net and its buffers
class Ctx(object):
    def __init__(self, name, max_batch):
        from xingtian_amd import lib as L
        from xingtian_amd.model.hip_net import HipActorCritic
        self.L, self.lib, self.name = L, L.load(), name
        self.spec, self.ospec = H.build_specs(name)
        self.net = HipActorCritic(self.spec, max_batch=max_batch, seed=0)
        self.params0 = H.seeded_params(name, self.ospec)
        self.net.set_weights({k: v.reshape(self.spec.names[k][1]) for k, v in self.params0.items()})
        self.flat0 = self.net.params.clone()
        self.data, self.acc = {}, {}
        self.frame = int(np.prod(H.NETS[name]["state_dim"]))      # uint8 bytes of one IMPALA frame

    # every run starts here: the saved parameters, a reset optimiser of the call's kind
    def reset(self, opt="adam"):
        self.net.params.copy_(self.flat0)
        self.net.touch()
        self.net.opt_kind = opt
        self.net.reset_optimizer()

    def rebind(self):
        """``xt_net_bind`` to the same buffers: the graphs go, the counters stay"""
        n = self.net
        self.L.check(self.lib.xt_net_bind(n.handle, self.L.ptr(n.params), self.L.ptr(n.grads), self.L.ptr(n.adam_m),
                                          self.L.ptr(n.adam_v), self.L.ptr(n.adam_state), self.L.ptr(n.workspace),
                                          n.workspace.numel() * 4), "xt_net_bind")

    def info(self):
        return self.net.graph_cache_info()

    def put_ppo(self, key, host):
        if key not in self.data:
            f32 = lambda a: _d(np.asarray(a, np.float32).reshape(-1))
            f64 = lambda a: _d(np.asarray(a, np.float64).reshape(-1))
            self.data[key] = dict(host=host, obs=self.net.to_device_obs(host["obs"]), perm=_d(host["perm"]),
                                  action=_d(host["action"]), old_logp=f32(host["old_logp"]), adv=f64(host["adv"]),
                                  old_v=f32(host["old_v"]), target_v=f64(host["target_v"]))
        return self.data[key]

    def put_impala(self, key, host):
        if key not in self.data:
            self.data[key] = dict(host=host, **{k: _d(v) for k, v in host.items()})
        return self.data[key]

    def loss_acc(self, key):
        if key not in self.acc:
            self.acc[key] = torch.zeros(8, dtype=torch.float32, device="cuda")
        return self.acc[key]

    def buf(self, call, what):
        return self.data[call[what]][what]


_CTX = {}


def ctx_of(name, max_batch):
    if (name, max_batch) not in _CTX:
        _CTX[(name, max_batch)] = Ctx(name, max_batch)
    return _CTX[(name, max_batch)]


def entry_of(call):
    return "impala" if "sample_batch_step" in call else "ppo"


def ctx_for(call):
    """the net of a mutation-table call with the data sets "A" and "B" resident"""
    ctx = ctx_of(call["net"], call["max_batch"])
    for i, key in enumerate("AB"):
        if entry_of(call) == "ppo":
            ctx.put_ppo(key, H.ppo_data(call["net"], H.PPO_DATA_ROWS, H.PPO_DATA_EPOCHS, 10 + i))
        else:
            ctx.put_impala(key, H.impala_data(call["net"], H.IMPALA_DATA_ROWS, H.IMPALA_DATA_CHUNKS, 10 + i))
    return ctx


# ------------------------------------------------------------------------------------------------ the raw calls
def ppo_cfg(ctx, call):
    c = ctx.L.PpoCfg()
    for f in H.PPO_CFG_FIELDS:
        setattr(c, f, call[f])
    return c


def impala_cfg(ctx, call):
    c = ctx.L.ImpalaCfg()
    for f in H.IMPALA_CFG_FIELDS:
        setattr(c, f, ctx.L.OPT_TYPE[call[f]] if f == "opt_type" else call[f])
    return c


def set_switches(ctx, call):
    net = ctx.net
    if entry_of(call) == "ppo":
        if net.train_stats_on != call["train_stats"]:
            net.set_train_stats(call["train_stats"])
        if net.gauss_fused_on != call["gauss_fused"]:
            net.set_gauss_fused(call["gauss_fused"])
    elif net.impala_stats_on != call["impala_stats"]:
        net.set_impala_stats(call["impala_stats"])


def enqueue(ctx, call, use_graph):
    """the train call of ``call`` through the raw binding -> its return code"""
    L, lib, net = ctx.L, ctx.lib, ctx.net
    set_switches(ctx, call)
    acc = ctx.loss_acc(call["loss_acc"])
    net.touch()
    if entry_of(call) == "ppo":
        c = ppo_cfg(ctx, call)
        return lib.xt_net_ppo_train(net.handle, ctypes.byref(c), L.ptr(ctx.buf(call, "obs")), call["n"],
                                    L.ptr(ctx.buf(call, "perm")), L.ptr(ctx.buf(call, "action")),
                                    L.ptr(ctx.buf(call, "old_logp")), L.ptr(ctx.buf(call, "adv")),
                                    L.ptr(ctx.buf(call, "old_v")), L.ptr(ctx.buf(call, "target_v")), L.ptr(acc),
                                    1 if use_graph else 0, L.stream_ptr())
    c = impala_cfg(ctx, call)
    lr = ctx.buf(call, "lr_steps") if call["lr_steps"] is not None else None
    return lib.xt_net_impala_train(net.handle, ctypes.byref(c), L.ptr(ctx.buf(call, "obs")), call["n"], call["batch_size"],
                                   L.ptr(ctx.buf(call, "bp_logits")), L.ptr(ctx.buf(call, "action")),
                                   L.ptr(ctx.buf(call, "done")), L.ptr(ctx.buf(call, "reward")), L.ptr(lr), L.ptr(acc),
                                   1 if use_graph else 0, L.stream_ptr())


def state(ctx, call):
    torch.cuda.synchronize()
    net = ctx.net
    s = dict(params=net.params.cpu().numpy(), m=net.adam_m.cpu().numpy(), v=net.adam_v.cpu().numpy(),
             adam_state=net.adam_state.cpu().numpy(), loss_acc=ctx.loss_acc(call["loss_acc"]).cpu().numpy()[:2])
    if call.get("train_stats"):
        s["stats"] = net._tstats["acc"].cpu().numpy()
    if call.get("impala_stats"):
        s["stats"] = net._istats["acc"].cpu().numpy()
    return s


def run(ctx, call, use_graph):
    """one train from the start state (the accumulator poisoned: the call clears it itself) -> the state it leaves"""
    ctx.reset(call.get("opt_type", "adam"))
    ctx.loss_acc(call["loss_acc"]).fill_(123.0)
    ctx.L.check(enqueue(ctx, call, use_graph), "train entry")
    return state(ctx, call)


def delta(after, before):
    return {k: after[k] - before[k] for k in ("captures", "launches", "evictions")}


# ------------------------------------------------------------------------------------------------ a, b: the loops
def ppo_loop_call(row):
    key = "loop:" + row["id"]
    ctx = ctx_of(row["net"], row["max_batch"])
    ctx.put_ppo(key, H.ppo_data(row["net"], row["n"], row["epochs"], row["seed"]))
    call = dict(H.PPO_CALL, net=row["net"], max_batch=row["max_batch"], n=row["n"], batch_size=row["batch"],
                num_sgd_iter=row["epochs"], global_batch=row["global_batch"], train_stats=row["stats"],
                gauss_fused=row["gauss_fused"], **{p: key for p in H.PPO_POINTERS})
    return ctx, call


def impala_loop_call(row):
    key = "loop:" + row["id"]
    ctx = ctx_of(row["net"], row["max_batch"])
    ctx.put_impala(key, H.impala_data(row["net"], row["n"], row["steps"], row["seed"]))
    call = dict(H.IMPALA_CALL, max_batch=row["max_batch"], n=row["n"], batch_size=row["batch_size"],
                sample_batch_step=row["T"], opt_type=row["opt"], impala_stats=row["stats"],
                **{p: key for p in H.IMPALA_POINTERS})
    if not row["lr_steps"]:
        call["lr_steps"] = None
    return ctx, call


_EAGER = {}


def eager(row, maker):
    """the eager train of a loop row, run once and shared by (a) and (b)"""
    if row["id"] not in _EAGER:
        ctx, call = maker(row)
        _EAGER[row["id"]] = run(ctx, call, False)
    return _EAGER[row["id"]]


@pytest.mark.parametrize("rid", H.PPO_LOOP_IDS)
def test_ppo_loop_is_bitwise_its_steps_composed_by_hand(rid):
    """``ppo_train_enqueue`` against ``xt_net_ppo_step(apply = 1)`` called by the test: rows ``perm[ep, start:start + B]``
    of every minibatch of the row's literal sizes, the ``global_batch`` the loop hands a short one, one ``loss_acc``."""
    row = H.PPO_LOOP[H.PPO_LOOP_IDS.index(rid)]
    ctx, call = ppo_loop_call(row)
    got = eager(row, ppo_loop_call)
    assert got["loss_acc"][1] == row["steps"]
    L, lib, net = ctx.L, ctx.lib, ctx.net
    ctx.reset()
    set_switches(ctx, call)
    acc = ctx.loss_acc(call["loss_acc"])
    acc.zero_()
    if row["stats"]:
        net.clear_train_stats()
    perm = ctx.buf(call, "perm")
    for ep in range(row["epochs"]):
        start = 0
        for b in row["sizes"]:
            c = ppo_cfg(ctx, dict(call, global_batch=H.ppo_step_global_batch(row["global_batch"], b, row["batch"])))
            L.check(lib.xt_net_ppo_step(net.handle, ctypes.byref(c), L.ptr(ctx.buf(call, "obs")),
                                        _at(perm, ep * row["n"] + start), b, L.ptr(ctx.buf(call, "action")),
                                        L.ptr(ctx.buf(call, "old_logp")), L.ptr(ctx.buf(call, "adv")),
                                        L.ptr(ctx.buf(call, "old_v")), L.ptr(ctx.buf(call, "target_v")), 1, None, L.ptr(acc),
                                        L.stream_ptr()), "xt_net_ppo_step")
            start += b
        assert start == row["n"]
    assert_same_state(got, state(ctx, call), rid)
    if row["stats"]:
        s = got["stats"]
        assert s[L.TRAIN_STATS_SLOTS["STEPS"]] == row["steps"] and s[L.TRAIN_STATS_SLOTS["ROWS"]] == row["n"] * row["epochs"]


@pytest.mark.parametrize("rid", H.PPO_LOOP_IDS)
def test_ppo_loop_against_float64(rid):
    row = H.PPO_LOOP[H.PPO_LOOP_IDS.index(rid)]
    ctx, call = ppo_loop_call(row)
    got = eager(row, ppo_loop_call)
    host = ctx.data[call["obs"]]["host"]
    cfg = dict(LR=call["lr"], LOSS_CLIPPING=call["clip_ratio"], ENTROPY_LOSS=call["ent_coef"], VF_CLIP=call["vf_clip"],
               CRITIC_LOSS_COEF=call["critic_coef"], MAX_GRAD_NORM=call["max_grad_norm"], BATCH_SIZE=row["batch"],
               NUM_SGD_ITER=row["epochs"])
    orc = nets.PpoLearnerOracle(ctx.ospec, {k: v.copy() for k, v in ctx.params0.items()}, cfg, np.float64)
    ref_loss = orc.train([host["obs"]], [host["action"], host["old_logp"], host["adv"], host["old_v"], host["target_v"]],
                         host["perm"])
    _check_float64(ctx, row, got, ref_loss, orc, call["lr"], "ppo")


def _check_float64(ctx, row, got, ref_loss, orc, lr, entry):
    loss = got["loss_acc"][0] / got["loss_acc"][1]
    loss_err = abs(loss - ref_loss) / max(1.0, abs(ref_loss))
    flat = got["params"]
    worst_abs, worst_rel = 0.0, 0.0
    for k, ref in orc.net.params.items():
        g = ctx.spec.var_view(flat, k).astype(np.float64).reshape(ref.shape)
        init = np.asarray(ctx.params0[k], np.float64).reshape(ref.shape)
        worst_abs = max(worst_abs, float(np.abs(g - ref).max()))
        worst_rel = max(worst_rel, H.rel_err(g - init, ref - init))
    bound = H.BARS["steps_lr"] * row["steps"] * lr
    print("PARITY {} {} steps={} loss_err={:.3g} (bar {:.0e}) max|dparam|={:.3g} (bar {:.3g}) rel_err(update)={:.3g}{}".format(
        entry, row["id"], row["steps"], loss_err, H.BARS["loss"], worst_abs, bound, worst_rel,
        " (bar {:.0e})".format(H.BARS["delta"]) if row["net"] in H.SMOOTH else " (relu: not held)"))
    assert loss_err < H.BARS["loss"], (loss, ref_loss)
    assert worst_abs <= bound, (worst_abs, bound)
    if row["net"] in H.SMOOTH:
        assert worst_rel < H.BARS["delta"], worst_rel


def _chunk_args(ctx, call, lo):
    """pointers of the chunk that starts at frame ``lo``"""
    a = H.NETS[call["net"]]["action_dim"]
    return (_at(ctx.buf(call, "obs"), lo * ctx.frame), _at(ctx.buf(call, "bp_logits"), lo * a),
            _at(ctx.buf(call, "action"), lo), _at(ctx.buf(call, "done"), lo), _at(ctx.buf(call, "reward"), lo))


@pytest.mark.parametrize("rid", H.IMPALA_LOOP_IDS)
def test_impala_loop_is_bitwise_its_chunks_composed_by_hand(rid):
    """``impala_train_enqueue`` against one eager ``xt_net_impala_train`` per chunk (``n`` = that chunk, ``lr_steps + i``),
    the chunk losses summed on the host in float32 in chunk order; without step sizes also against
    ``xt_net_impala_step(apply = 1)`` per chunk into one ``loss_acc``."""
    row = H.IMPALA_LOOP[H.IMPALA_LOOP_IDS.index(rid)]
    ctx, call = impala_loop_call(row)
    got = eager(row, impala_loop_call)
    assert got["loss_acc"][1] == row["steps"]
    L, lib, net = ctx.L, ctx.lib, ctx.net
    c = impala_cfg(ctx, call)
    acc = ctx.loss_acc(call["loss_acc"])
    # ---- one train per chunk
    ctx.reset(row["opt"])
    set_switches(ctx, call)
    total, count, lo = np.float32(0.0), np.float32(0.0), 0
    for i, nfr in enumerate(row["sizes"]):
        acc.fill_(123.0)
        lr = _at(ctx.buf(call, "lr_steps"), i) if row["lr_steps"] else None
        o, bp, act, done, rew = _chunk_args(ctx, call, lo)
        L.check(lib.xt_net_impala_train(net.handle, ctypes.byref(c), o, nfr, call["batch_size"], bp, act, done, rew, lr,
                                        L.ptr(acc), 0, L.stream_ptr()), "xt_net_impala_train")
        a = acc.cpu().numpy()
        assert a[1] == 1.0
        total, count = np.float32(total + a[0]), np.float32(count + a[1])
        lo += nfr
    assert lo == row["n"]
    ref = state(ctx, call)
    ref["loss_acc"] = np.array([total, count], np.float32)
    if row["stats"]:
        # every per-chunk train clears the statistics at its start: the whole call's sums are the step composition's
        # business (below); the two counters are held here
        s = got["stats"]
        assert s[L.IMPALA_STATS_SLOTS["CHUNKS"]] == row["steps"]
        assert s[L.IMPALA_STATS_SLOTS["TRANSITIONS"]] == row["n"] - row["n"] // row["T"]
        ref["stats"] = got["stats"]
    assert_same_state(got, ref, rid + " / train per chunk")
    if row["lr_steps"]:
        return
    # ---- one step per chunk
    ctx.reset(row["opt"])
    acc.zero_()
    if row["stats"]:
        net.clear_impala_stats()
    lo = 0
    for nfr in row["sizes"]:
        o, bp, act, done, rew = _chunk_args(ctx, call, lo)
        L.check(lib.xt_net_impala_step(net.handle, ctypes.byref(c), o, nfr, bp, act, done, rew, 1, L.ptr(net.loss_out),
                                       L.ptr(acc), L.stream_ptr()), "xt_net_impala_step")
        lo += nfr
    assert_same_state(got, state(ctx, call), rid + " / step per chunk")


@pytest.mark.parametrize("rid", H.IMPALA_LOOP_IDS)
def test_impala_loop_against_float64(rid):
    row = H.IMPALA_LOOP[H.IMPALA_LOOP_IDS.index(rid)]
    ctx, call = impala_loop_call(row)
    got = eager(row, impala_loop_call)
    host = ctx.data[call["obs"]]["host"]
    cfg = dict(LR=call["lr"], grad_norm_clip=call["grad_norm_clip"], sample_batch_step=row["T"], BATCH_SIZE=row["batch_size"],
               GAMMA=call["gamma"], opt_type=row["opt"])
    orc = nets.ImpalaLearnerOracle(ctx.ospec, {k: v.copy() for k, v in ctx.params0.items()}, cfg, np.float64)
    losses, lo, lr_max = [], 0, 0.0
    for i, nfr in enumerate(row["sizes"]):
        lr = float(host["lr_steps"][i]) if row["lr_steps"] else call["lr"]
        orc.opt.lr = lr
        lr_max = max(lr_max, lr)
        sl = slice(lo, lo + nfr)
        losses.append(orc.step(host["obs"][sl], host["bp_logits"][sl], host["action"][sl], host["done"][sl].astype(bool),
                               host["reward"][sl])["loss"])
        lo += nfr
    _check_float64(ctx, row, got, float(np.mean(losses)), orc, lr_max, "impala")


# ------------------------------------------------------------------------------------------------ c: replay under mutation
@pytest.mark.parametrize("mid", H.MUTATION_IDS)
def test_replay_is_the_eager_call_after_every_change(mid):
    """graph(base), graph(mutated), graph(base) on one net: the second is eager(mutated), the third eager(base), bit for
    bit; a live mutation changes the parameters (a stale replay cannot pass); two captures, three launches."""
    row = H.MUTATIONS[H.MUTATION_IDS.index(mid)]
    base, mut = H.call_of(row, False), H.call_of(row, True)
    ctx = ctx_for(base)
    ctx.rebind()
    assert ctx.info()["live_slots"] == 0
    before = ctx.info()
    e_base, e_mut = run(ctx, base, False), run(ctx, mut, False)
    assert delta(ctx.info(), before) == dict(captures=0, launches=0, evictions=0)
    if row["live"]:
        assert not same(e_base["params"], e_mut["params"]), "the mutation leaves the same parameters: the row tests nothing"
    assert_same_state(run(ctx, base, True), e_base, mid + " / graph(base)")
    assert_same_state(run(ctx, mut, True), e_mut, mid + " / graph(mutated)")
    assert_same_state(run(ctx, base, True), e_base, mid + " / graph(base) again")
    after = ctx.info()
    assert delta(after, before) == dict(captures=2, launches=3, evictions=0), (after, before)
    assert after["live_slots"] == 2


# ------------------------------------------------------------------------------------------------ d: same key, new contents
@pytest.mark.parametrize("entry", ["ppo", "impala"])
def test_one_graph_follows_the_contents_of_its_buffers(entry):
    call = dict(H.PPO_CALL) if entry == "ppo" else dict(H.IMPALA_CALL, lr_steps="A")
    ctx = ctx_for(call)
    src = ctx.data["B"]
    put = ctx.put_ppo if entry == "ppo" else ctx.put_impala
    if entry == "ppo":
        work = put("D", H.ppo_data(call["net"], H.PPO_DATA_ROWS, H.PPO_DATA_EPOCHS, 10))
        order = ("perm", "action", "old_logp", "adv", "old_v", "target_v", "obs")
    else:
        work = put("D", H.impala_data(call["net"], H.IMPALA_DATA_ROWS, H.IMPALA_DATA_CHUNKS, 10))
        order = ("bp_logits", "action", "done", "reward", "obs", "lr_steps")
    for p in order:
        work[p].copy_(ctx.data["A"][p])           # (an earlier run of this test may have left other contents)
        call[p] = "D"
    ctx.rebind()
    before = ctx.info()
    flat0 = ctx.flat0
    try:
        assert_same_state(run(ctx, call, True), run(ctx, call, False), entry + " / first")
        seen = [run(ctx, call, False)["params"]]
        for p in order + ("params",):
            if p == "params":
                other = H.seeded_params(call["net"], ctx.ospec, seed=1)
                ctx.net.set_weights({k: v.reshape(ctx.spec.names[k][1]) for k, v in other.items()})
                ctx.flat0 = ctx.net.params.clone()
            else:
                work[p].copy_(src[p])
            want = run(ctx, call, False)
            assert not any(same(want["params"], s) for s in seen), (entry, p, "the new contents change nothing")
            seen.append(want["params"])
            assert_same_state(run(ctx, call, True), want, entry + " / new " + p)
        assert delta(ctx.info(), before) == dict(captures=1, launches=len(order) + 2, evictions=0)
    finally:
        ctx.flat0 = flat0


# ------------------------------------------------------------------------------------------------ e: eviction
def test_ninth_key_evicts_the_least_recently_used_graph():
    ctx = ctx_for(H.PPO_CALL)
    ctx.rebind()
    want = run(ctx, H.PPO_CALL, False)
    key = lambda i: dict(H.PPO_CALL, loss_acc="K%d" % i)
    slots = ctx.L.GRAPH_CACHE_SLOTS
    before = ctx.info()

    def graph(i, captures, evictions):
        """run key i through the cache: bitwise the eager call, and the counters move as said"""
        b = ctx.info()
        assert_same_state(run(ctx, key(i), True), want, "key %d" % i)
        a = ctx.info()
        assert (a["captures"] - b["captures"], a["evictions"] - b["evictions"], a["launches"] - b["launches"]) == \
            (captures, evictions, 1), (i, a, b)

    for i in range(slots):
        graph(i, 1, 0)
    graph(slots, 1, 1)                       # the ninth key: key 0 goes
    assert delta(ctx.info(), before) == dict(captures=slots + 1, launches=slots + 1, evictions=1)
    assert ctx.info()["live_slots"] == slots
    graph(0, 1, 1)                           # the first key again: a capture, key 1 goes
    assert delta(ctx.info(), before) == dict(captures=slots + 2, launches=slots + 2, evictions=2)
    assert ctx.info()["live_slots"] == slots
    for i in range(2, slots + 1):            # touch keys 3..9: the first key is now the least recently used
        graph(i, 0, 0)
    graph(slots + 1, 1, 1)                   # a new key: the first key goes ...
    graph(2, 0, 0)                           # ... key 3 is still there
    graph(0, 1, 1)                           # ... and the first key is not
    assert ctx.info()["live_slots"] == slots


# ------------------------------------------------------------------------------------------------ f: interleaving, rebind
@pytest.mark.parametrize("entry", ["ppo", "impala"])
def test_eager_and_graph_calls_interleave_and_a_rebind_empties_the_cache(entry):
    a = dict(H.PPO_CALL if entry == "ppo" else H.IMPALA_CALL)
    b = dict(a, lr=1e-3, obs="B")
    ctx = ctx_for(a)
    ctx.rebind()
    before = ctx.info()
    ea = run(ctx, a, False)
    assert_same_state(run(ctx, a, True), ea, "graph A")
    eb = run(ctx, b, False)
    assert not same(ea["params"], eb["params"])
    assert_same_state(run(ctx, b, True), eb, "graph B")
    assert_same_state(run(ctx, a, True), ea, "graph A again")
    assert_same_state(run(ctx, a, False), ea, "eager A again")
    assert delta(ctx.info(), before) == dict(captures=2, launches=3, evictions=0)
    assert ctx.info()["live_slots"] == 2
    # fresh buffers: every graph holds the old addresses, so the bind destroys them all
    net = ctx.net
    old = (net.params, net.grads_xchg, net.grads, net.adam_m, net.adam_v, net.adam_state, net.workspace)
    try:
        net.params, net.grads_xchg = net.params.clone(), torch.zeros_like(net.grads_xchg)
        net.grads = net.grads_xchg[:net.params.numel()]
        net.adam_m, net.adam_v, net.adam_state = net.adam_m.clone(), net.adam_v.clone(), net.adam_state.clone()
        net.workspace = torch.empty_like(net.workspace)
        ctx.rebind()
        assert ctx.info()["live_slots"] == 0
        mid = ctx.info()
        assert_same_state(run(ctx, a, True), ea, "graph A on the new buffers")
        assert delta(ctx.info(), mid) == dict(captures=1, launches=1, evictions=0)
        assert_same_state(run(ctx, a, False), ea, "eager A on the new buffers")
    finally:
        torch.cuda.synchronize()
        (net.params, net.grads_xchg, net.grads, net.adam_m, net.adam_v, net.adam_state, net.workspace) = old
        ctx.rebind()


# ------------------------------------------------------------------------------------------------ g: refusals
REFUSALS = [
    ("ppo", "n=0", dict(n=0)),
    ("ppo", "batch_size>maxB", dict(batch_size=9)),
    ("ppo", "num_sgd_iter=0", dict(num_sgd_iter=0)),
    ("ppo", "shard_world=2,no_hook", dict(shard_world=2)),              # refused INSIDE the capture
    ("ppo", "shard_world=2,no_hook,stats", dict(shard_world=2, train_stats=True)),      # ... behind two captured nodes
    ("impala", "n=0", dict(n=0)),
    ("impala", "n%T", dict(n=15)),
    ("impala", "batch_size%T", dict(batch_size=15)),
    ("impala", "batch_size>maxB,n>maxB", dict(batch_size=40)),
    ("impala", "shard_world=2,no_hook", dict(shard_world=2)),           # inside the capture, nothing enqueued yet
    ("impala", "shard_world=2,no_hook,stats", dict(shard_world=2, impala_stats=True)),  # ... behind the statistics' clear
]


@pytest.mark.parametrize("entry,what,bad", REFUSALS, ids=["%s:%s" % r[:2] for r in REFUSALS])
def test_a_refused_call_returns_an_error_and_leaves_the_net_usable(entry, what, bad):
    good = dict(H.PPO_CALL if entry == "ppo" else H.IMPALA_CALL)
    ctx = ctx_for(good)
    ctx.rebind()
    want = run(ctx, good, False)
    before = ctx.info()
    ctx.reset()
    rc = enqueue(ctx, dict(good, **bad), True)
    msg = ctx.lib.xt_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and ("xt_net_ppo_train" if entry == "ppo" else "xt_net_impala_train") in msg, (rc, msg)
    after = ctx.info()
    assert after["live_slots"] == before["live_slots"] == 0
    assert delta(after, before) == dict(captures=0, launches=0, evictions=0)
    assert_same_state(run(ctx, good, True), want, what + " / the next graph call")
    assert_same_state(run(ctx, good, True), want, what + " / its replay")
    assert delta(ctx.info(), before) == dict(captures=1, launches=2, evictions=0)
