"""CPU tests (no GPU) of the SCC learner: the registry and the CPU agent, the layout arithmetic against the library, every refusal
with its message, the C ABI table against the header, and the identity the credits kernel rests on."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import scc_helpers as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# examples/ma_cases/scc.yaml's model_config, with what the algorithm adds from the 2s_vs_1sc environment
EXAMPLE = dict(gamma=0.99, c_lr=0.0005, a_lr=0.0005, mixer_grad_norm_clip=10, actor_grad_norm_clip=10, rnn_hidden_dim=64, batch_size=32,
               use_double_q=True, dense_unit_number=128, enable_critic_multi_channel=True, channel_merge="concat", mc_sample_times=3,
               map_name="2s_vs_1sc", n_agents=2, n_actions=7, obs_shape=26, state_shape=27, episode_limit=300)


def test_registry_layout_and_the_cpu_agent():
    from xingtian_amd import lib as L
    from xingtian_amd.model import model_builder
    m = model_builder(dict(model_name="SCCModel", model_config=dict(EXAMPLE, SEED=3)))
    assert type(m).__name__ == "SCCModel" and m.net.inference_only and m.agent_group == [2] and m.spec.o == 17
    assert m.infer_actions(np.zeros((1, 1, 2, 26), np.float32)).shape == (1, 2, 7) and len(m.get_weights()) == 8
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train(*[None] * 10)
    spec = S.SCCSpec(dict(EXAMPLE, map_name="2s3z", n_agents=5, obs_shape=29, channel_merge="add"))
    assert spec.groups == [2, 3] and list(spec.names)[8:13] == ["mixer/group0/layer_1/kernel", "mixer/group0/layer_1/bias",
                                                                  "mixer/group0/layer_2/kernel", "mixer/group0/layer_2/bias",
                                                                  "mixer/group1/layer_1/kernel"]
    assert spec.names["mixer/group1/layer_1/kernel"][1] == (24, 128) and spec.names["mixer/v/kernel"][1] == (128, 1)
    assert m.spec.names["mixer/v/kernel"][1] == (256, 1)
    offs, nt = (ctypes.c_int64 * (L.SCC_MAX_TENSORS + 1))(), ctypes.c_int32()
    assert L.load().xt_scc_layout(ctypes.byref(spec.desc(L)), offs, ctypes.byref(nt)) == 0 and nt.value == 18
    assert list(offs[:19]) == [o for o, _ in spec.names.values()] + [spec.n_flat] and offs[8] == spec.n_agent_flat


@pytest.mark.parametrize("over,desc,word", [
    (dict(enable_critic_multi_channel=False), dict(multi_channel=0), "enable_critic_multi_channel = False"),
    (dict(dense_unit_number=48), dict(units=48), "dense_unit_number = 48 (the critic kernels take 32, 64 or 128)"),
    (dict(obs_shape=1100), dict(obs_dim=1100), "o + n_actions = 1098 above 1024"),
    (dict(rnn_hidden_dim=48), dict(hidden=48), "rnn_hidden_dim = 48 (the recurrent kernels take 32 or 64)"),
    (dict(n_agents=33, obs_shape=60), dict(n_agents=33, obs_dim=60), "n_agents = 33"),
    (dict(n_actions=65, obs_shape=90), dict(n_actions=65, obs_dim=90), "n_actions = 65"),
    (dict(channel_merge="mul"), dict(merge=2), "is neither concat nor add"),
    (dict(agent_group=[1, 2]), dict(n_groups=2, groups=(1, 2)), "agent_group sums to 3, n_agents = 2"),
    (dict(allow_mix_precision=True), None, "allow_mix_precision")])
def test_refusals_on_the_host(over, desc, word):
    """the model refuses, and the library refuses with the same words before any device call (nothing is launched here)"""
    from xingtian_amd import lib as L
    with pytest.raises(ValueError, match=re.escape(word)):
        S.SCCSpec(dict(EXAMPLE, **over))
    if desc is not None:
        d = S.SCCSpec(EXAMPLE).desc(L)
        for k, v in desc.items():
            setattr(d, k, (ctypes.c_int32 * 32)(*v) if k == "groups" else v)
        h = ctypes.c_void_p()
        assert L.load().xt_scc_create(ctypes.byref(d), 4, ctypes.byref(h)) != 0 and not h.value
        assert word in L.load().xt_last_error().decode()


def test_double_q_off_raises_as_the_reference():
    with pytest.raises(RuntimeError, match="double q is needed"):
        S.SCCSpec(dict(EXAMPLE, use_double_q=False))


def test_abi_symbols_are_declared_in_header_and_table():
    from xingtian_amd import lib as L
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    section = header[header.index("SCC: GRU agents, the multi-channel critic"):]
    declared = set(re.findall(r"^(?:int|void|int64_t) (xt_scc_[a-z_]+)\(", section, re.M))
    assert declared == {k for k in L.SIGNATURES if k.startswith("xt_scc_")} and len(declared) == 10
    for name in sorted(declared):
        args = re.search(r"\b(?:int|void|int64_t) %s\(([^;]*)\);" % name, section).group(1).split(",")
        assert len(L.SIGNATURES[name][1]) == len(args) and getattr(L.load(), name), name
    assert ctypes.sizeof(L.SccDesc) == 4 * (9 + L.SCC_MAX_GROUPS) and ctypes.sizeof(L.SccCfg) == 40
    for word, val in (("MAX_GROUPS", L.SCC_MAX_GROUPS), ("MAX_TENSORS", L.SCC_MAX_TENSORS), ("STATE_FLOATS", L.SCC_STATE_FLOATS)):
        assert int(re.search(r"#define XT_SCC_%s (\d+)" % word, header).group(1)) == val


@pytest.mark.parametrize("merge", ["concat", "add"])
def test_credits_do_not_depend_on_the_draws(merge):
    """the critic is additive over the agents: whatever coalitions ``random`` draws, credit i is w_i . (h_i(full) - h_i(action
    part zeroed)) up to rounding: two seeds agree to 1e-10 of the largest credit, and both equal the closed form"""
    spec = S.make_spec(n=3, groups=[1, 2], merge=merge)
    params, case = S.make_params(spec, 5), S.make_case(spec, 3, 50)
    p = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in params.items()}
    x = torch.as_tensor(S.critic_state(spec, case["obs"], case["actions"]))
    v_of = lambda y: S.critic_ref(spec, p, "eval_mixer", y)      # noqa: E731
    c1, c2 = (S.credits_ref(spec, v_of, x, 3, random.Random(seed)).numpy() for seed in (1, 2))
    closed = []
    for i in range(3):
        m = torch.ones_like(x)
        m[:, :, i * 8 + 5:(i + 1) * 8] = 0
        closed.append((v_of(x) - v_of(m * x))[..., 0].numpy())
    scale = np.abs(c1).max()
    print("seed 1 vs 2: {:.3e}, vs the closed form: {:.3e}".format(np.abs(c1 - c2).max() / scale, np.abs(c1 - np.stack(closed, 2)).max() / scale))
    assert scale > 1e-3 and np.abs(c1 - c2).max() <= 1e-10 * scale and np.abs(c1 - np.stack(closed, 2)).max() <= 1e-10 * scale

