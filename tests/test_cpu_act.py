"""CPU tests of the device acting path (``PREDICT_ON_DEVICE`` / ``xt_net_act``): the numpy restatement of its generator
against known answers, the sampling law of that restatement, the configuration key on the CPU replica, and the two new
C-ABI symbols with their struct."""
import ctypes
import os
import re

import numpy as np
import pytest

import act_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _module_constants_restored():
    """import_config overrides the model modules' constants for the rest of the process: put them back"""
    from xingtian_amd.model.impala import impala_cnn_opt
    from xingtian_amd.model.ppo import ppo
    saved = [(m, {k: v for k, v in vars(m).items() if k.isupper()}) for m in (ppo, impala_cnn_opt)]
    yield
    for m, consts in saved:
        vars(m).update(consts)


def test_philox_restatement_known_answers():
    hexs = lambda w: " ".join("%08x" % x for x in w)
    f = 0xFFFFFFFF
    assert hexs(H.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexs(H.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    # the third vector of the generator's published known-answer set (digits of pi)
    assert hexs(H.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # arrays go through word by word
    w = H.philox4x32_10((np.array([0, f]), np.array([0, f]), np.array([0, f]), np.array([0, f])), (0, 0))
    assert w.shape == (2, 4) and hexs(w[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"


def test_word_to_uniform_never_reaches_zero_or_one():
    u = H.uniform([0, 0xFFFFFFFF])
    assert u[0] == 2.0 ** -24 and u[1] == 1.0 - 2.0 ** -24
    # the same steps in float32 are exact: (w >> 9) < 2^23, + 0.5 fits 24 bits, the scale is a power of two
    w = np.array([0, 1 << 9, 0x80000000, 0xFFFFFFFF], np.uint32)
    u32 = ((w >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert u32.dtype == np.float32 and np.array_equal(u32.astype(np.float64), H.uniform(w))
    assert 0.0 < u32.min() and u32.max() < 1.0


def test_layout_of_the_draws():
    """action k of row r: word k & 3 of block (r, k >> 2, call); dimension k: words 2(k & 1), 2(k & 1) + 1 of block k >> 1"""
    seed, call = (0x12345678 << 32) | 0x9ABCDEF0, (7 << 32) | 3
    u = H.categorical_uniforms(seed, call, [5, 70000], 6)
    w = H.philox4x32_10((70000, 1, 3, 7), (0x9ABCDEF0, 0x12345678))
    assert u.shape == (2, 6) and u[1, 5] == H.uniform(w[1]) and u[1, 4] == H.uniform(w[0])
    e = H.gauss_eps(seed, call, [5, 70000], 3)
    u1, u2 = H.uniform(w[0]), H.uniform(w[1])          # dimension 2 = block 1, words 0 and 1
    assert e[1, 2] == np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


@pytest.mark.parametrize("case", range(3))
def test_categorical_sampling_law_of_the_restatement(case):
    logits = H.LAW_LOGITS[case]
    g = H.gumbel(H.LAW_SEED, H.LAW_CALL, np.arange(H.LAW_N), len(logits))
    action = np.argmax(logits[None, :] + g.astype(np.float32), axis=1)
    sig = H.categorical_law_sigmas(action, logits)
    print("A = %d: largest deviation %.2f sigma" % (len(logits), sig.max()))
    assert (sig <= 5.0).all()


def test_gaussian_sampling_law_of_the_restatement():
    sig = H.gauss_law_sigmas(H.gauss_eps(H.LAW_SEED, H.LAW_CALL, np.arange(H.LAW_N), 3))
    print("mean %.2f, variance %.2f, correlation %.2f sigma" % sig)
    assert max(sig) <= 5.0


def _same(a, b):
    return all(np.array_equal(x, y) and np.asarray(x).dtype == np.asarray(y).dtype and np.shape(x) == np.shape(y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("which", ["PpoMlp", "PpoMlpGauss", "ImpalaCnnOpt"])
def test_key_on_a_cpu_replica_leaves_predict_unchanged(which):
    """an explorer without a GPU reads the same YAML: the key is ignored silently"""
    from xingtian_amd.model import model_builder
    rng = np.random.default_rng(3)
    if which == "ImpalaCnnOpt":
        info = {"model_name": "ImpalaCnnOpt", "state_dim": [42, 42, 4], "action_dim": 6, "input_dtype": "uint8"}
        obs = rng.integers(0, 256, (3, 42, 42, 4)).astype(np.uint8)
    else:
        info = {"model_name": "PpoMlp", "state_dim": [4], "action_dim": 2}
        obs = rng.standard_normal((5, 4)).astype(np.float32)
    base = {"SEED": 5, "DEVICE": "cpu"}
    if which == "PpoMlpGauss":
        base["action_type"] = "DiagGaussian"
    plain = model_builder(dict(info, model_config=dict(base)))
    keyed = model_builder(dict(info, model_config=dict(base, PREDICT_ON_DEVICE=True)))
    assert keyed.net.inference_only and keyed._act is None and plain._act is None
    for _ in range(3):
        assert _same(plain.predict(obs), keyed.predict(obs))


def _header_struct(name):
    src = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    body = src[src.index("typedef struct %s {" % name):src.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(u?int\d+_t|float|double)\s+([\w\s,]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_header_signatures_and_struct_of_the_new_symbols():
    from xingtian_amd import lib
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    declared = set(re.findall(r"\b(xt_[a-z0-9_]+)\s*\(", header))
    for name, nargs in (("xt_net_act", 12), ("xt_act_heads", 18)):
        assert name in declared and name in lib.SIGNATURES
        assert len(lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib.load(), name)
    assert lib.load().xt_abi_version() == 12          # appended under ABI 12
    ctype_of = {"uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    fields = _header_struct("xt_act_cfg")
    assert [n for n, _ in fields] == ["seed", "call", "row0", "want_noise"]
    assert [(n, ctype_of[t]) for n, t in fields] == list(lib.ActCfg._fields_)
    assert ctypes.sizeof(lib.ActCfg) == 32 and lib.ActCfg.row0.offset == 16 and lib.ActCfg.want_noise.offset == 24
