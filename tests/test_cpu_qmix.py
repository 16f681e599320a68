"""CPU tests (no GPU) of the QMIX learner: the C ABI table against the header, the registry, the example's model_config, every
refusal with its message, the NumPy replica of the agent against float64, and the conditions the GPU tests put on their inputs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import qmix_helpers as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# examples/ma_cases/qmix.yaml's model_config, with what QMixAlg adds from the 2s_vs_1sc environment
EXAMPLE = dict(gamma=0.99, grad_norm_clip=10, hypernet_embed=64, hypernet_layers=2, lr=0.0005, mixing_embed_dim=32, rnn_hidden_dim=64,
               batch_size=32, use_double_q=True, n_agents=2, n_actions=7, obs_shape=26, state_shape=27, episode_limit=300)


def test_abi_stays_12_and_the_table_matches_the_header():
    from xingtian_amd import lib as L
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    assert re.search(r"#define XT_ABI_VERSION 12\b", header) and L.ABI_VERSION == 12
    section = header[header.index("QMIX: GRU agents and the monotonic mixer"):]
    declared = set(re.findall(r"^(?:int|void|int64_t) (xt_qmix_[a-z_]+)\(", section, re.M))
    assert declared == {k for k in L.SIGNATURES if k.startswith("xt_qmix_")} and len(declared) == 12
    handle = L.load()
    for name in sorted(declared):
        args = re.search(r"\b(?:int|void|int64_t) %s\(([^;]*)\);" % name, section).group(1).split(",")
        assert len(L.SIGNATURES[name][1]) == len(args) and getattr(handle, name), name
    for struct, cls in (("xt_qmix_desc", L.QmixDesc), ("xt_qmix_cfg", L.QmixCfg)):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        assert re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S)) == [n for n, _ in cls._fields_]
    assert int(re.search(r"#define XT_QMIX_TENSORS (\d+)", header).group(1)) == L.QMIX_TENSORS
    assert int(re.search(r"#define XT_QMIX_STATE_FLOATS (\d+)", header).group(1)) == L.QMIX_STATE_FLOATS


def test_registry_and_the_example_config(tmp_path):
    from xingtian_amd.model import model_builder
    from xingtian_amd.register import Registers
    assert Registers.model["QMixModel"].__name__ == "QMixModel"
    m = model_builder(dict(model_name="QMixModel", allow_mix_precision=True, model_config=dict(EXAMPLE, SEED=3)))
    assert m.net.inference_only and m.g_type == "explore"
    shapes = m.spec.tf_shapes()
    assert len(shapes) == 22 and list(shapes)[2] == "eval_agent/rnn/gru_cell/gates/kernel"
    want = [(26, 64), (64,), (128, 128), (128,), (128, 64), (64,), (64, 7), (7,), (27, 64), (64,), (64, 64), (64,), (27, 32), (32,),
            (27, 64), (64,), (64, 32), (32,), (27, 32), (32,), (32, 1), (1,)]
    assert list(shapes.values()) == want
    w = m.get_weights()
    assert list(w)[0] == "explore_agent/dense/kernel" and len(w) == 8 and (w["explore_agent/rnn/gru_cell/gates/bias"] == 1).all()
    assert m.infer_actions(np.zeros((1, 1, 2, 26), np.float32)).shape == (1, 2, 7) and m.hi_out_val.shape == (2, 64)
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train(*[None] * 9)
    # checkpoints: the explore agent's variables as .npz, under the reference's method names
    m.save_explore_agent_weights(str(tmp_path / "actor00001"))
    other = model_builder(dict(model_name="QMixModel", model_config=dict(EXAMPLE, SEED=4)))
    other.restore_explorer_variable(str(tmp_path / "actor00001"))
    assert all(np.array_equal(v, other.get_weights()[k]) for k, v in w.items())
    # the library lays a parameter set out as the model does (host arithmetic)
    from xingtian_amd import lib as L
    d = L.QmixDesc(n_agents=2, obs_dim=26, hidden=64, n_actions=7, state_dim=27, embed=32, hyper_embed=64, seq_len=300, double_q=1)
    offs = (ctypes.c_int64 * 23)()
    assert L.load().xt_qmix_layout(ctypes.byref(d), offs) == 0
    assert list(offs) == [o for o, _ in m.spec.names.values()] + [m.spec.n_flat] and offs[8] == m.spec.n_agent_flat


@pytest.mark.parametrize("over,word", [(dict(hidden=48), "rnn_hidden_dim = 48 (the recurrent kernels take 32 or 64)"),
                                       (dict(n_agents=33), "n_agents = 33"), (dict(n_actions=65), "n_actions = 65"),
                                       (dict(embed=65), "mixing_embed_dim = 65")])
def test_refusals_on_the_host(over, word):
    """the library refuses before any device call (nothing is launched here), and the model refuses with the same words"""
    from xingtian_amd import lib as L
    from xingtian_amd.model.qmix.qmix_model import QMixSpec
    lib = L.load()
    base = dict(n_agents=2, obs_dim=11, hidden=32, n_actions=5, state_dim=7, embed=8, hyper_embed=16, seq_len=4, double_q=1)
    h = ctypes.c_void_p()
    assert lib.xt_qmix_create(ctypes.byref(L.QmixDesc(**dict(base, **over))), 4, ctypes.byref(h)) != 0 and not h.value
    assert word in lib.xt_last_error().decode()
    (k, v), = over.items()
    with pytest.raises(ValueError, match=re.escape(word)):
        QMixSpec(dict(EXAMPLE, **{dict(hidden="rnn_hidden_dim", embed="mixing_embed_dim").get(k, k): v}))
    p = ctypes.c_void_p(4096)
    if "hidden" in over:
        assert lib.xt_qmix_gru_fwd(p, p, p, None, None, 2, 4, 48, None, p, None, None) != 0
        assert lib.xt_qmix_gru_bwd(p, p, p, None, p, None, None, 2, 4, 48, p, None, None) != 0 and word in lib.xt_last_error().decode()
    else:
        n, a, e = over.get("n_agents", 2), over.get("n_actions", 5), over.get("embed", 8)
        assert lib.xt_qmix_mix(p, p, p, p, p, p, p, p, p, 2, 2, n, a, e, 0.99, 1, p, p, None, p, p, None, None) != 0
        assert word in lib.xt_last_error().decode()


@pytest.mark.parametrize("h", [32, 64])
def test_numpy_replica_matches_float64(h):
    from xingtian_amd.model.qmix.qmix_model import CpuQmixAgent
    spec = Q.make_spec(n=3, h=h, t=5)
    net = CpuQmixAgent(spec, seed=h)
    rng = np.random.default_rng(h)
    net.set_weights({k: v + rng.uniform(-0.1, 0.1, v.shape).astype(np.float32) for k, v in net.get_weights().items()})
    obs = rng.standard_normal((2, 6, 3, spec.D)).astype(np.float32)
    lens = np.array([6, 0, 3, 6, 1, 5])
    q, hid = net.agent_forward(obs, np.zeros((6, h), np.float32), lens)
    p = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in net.get_weights().items()}
    q64, h64 = Q.agent_ref(p, "explore_agent", torch.as_tensor(obs, dtype=torch.float64), torch.as_tensor(lens))
    assert Q.rel(q, q64.numpy()) < 1e-5 and Q.rel(hid, h64.numpy()) < 1e-5
    assert np.array_equal(q[0, :, 1], np.broadcast_to(net.get_weights()["explore_agent/dense_1/bias"], (6, spec.A)))      # length 0: q = b2


def test_conditions_on_the_gpu_tests_inputs():
    """what tests/test_gpu_qmix.py relies on, checked on the float64 reference alone: arg-max gaps above 1e-4, sum(mask) > 0,
    the bars are the standing ones or four times the float32 restatement's deviation"""
    for b, n, t in Q.STEP_CASES:
        spec, params, case = Q.step_inputs(b, n, t)
        assert Q.step_ref(spec, params, case)[2] > 1e-4 and case["mask"].sum() > 0, (b, n, t)
    for k, (dev, bar) in Q.bars().items():
        print("{}: float32 restatement {:.3e}, bar {:.3e}".format(k, dev, bar))
        assert bar == max(Q.LOSS_BAR if k == "step_loss" else Q.GRAD_BAR, 4 * dev)
