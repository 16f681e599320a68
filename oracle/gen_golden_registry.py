"""Oracle (test infrastructure): what the reference's OWN plugin registry does with the HIP plugin classes.

zeus/common/util/register.py is loaded unmodified from a checkout of the reference (its two imports that need
uninstalled packages are stubbed: ``absl.logging`` -> stdlib logging and ``zeus.set_backend``, which would import
TensorFlow, -> no-op).  Drop-in subclasses of the four plugin classes are registered with its decorators, as
INTEGRATION.md section 1 tells a user to, and what the registry resolves -- plus how it treats a non-callable, an
unknown name, a second registration under one name and an attempt to instantiate ``Registers`` -- is committed as
tests/golden/registry.json, so that the test reads no reference file.

Usage:  python oracle/gen_golden_registry.py <reference checkout>
"""
import importlib.util
import json
import logging as pylogging
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "registry.json")
KINDS = ("agent", "model", "algorithm", "env", "comm")


def load_reference_registry(ref):
    absl = types.ModuleType("absl")
    absl.logging = pylogging
    zeus = types.ModuleType("zeus")
    zeus.set_backend = lambda **kw: None
    saved = {k: sys.modules.get(k) for k in ("absl", "absl.logging", "zeus")}
    sys.modules["absl"], sys.modules["absl.logging"], sys.modules["zeus"] = absl, pylogging, zeus
    try:
        spec = importlib.util.spec_from_file_location("_ref_register", os.path.join(ref, "zeus/common/util/register.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def plugin_subclasses():
    """The four drop-in subclasses, named as INTEGRATION.md section 1 names them: (kind, class)."""
    sys.path.insert(0, ROOT)
    from xingtian_amd.algorithm.impala.impala_opt import IMPALAOpt
    from xingtian_amd.algorithm.ppo.ppo import PPO
    from xingtian_amd.model.impala.impala_cnn_opt import ImpalaCnnOpt
    from xingtian_amd.model.ppo.ppo_cnn import PpoCnn
    return [("model", type("PpoCnnHip", (PpoCnn,), {})), ("model", type("ImpalaCnnOptHip", (ImpalaCnnOpt,), {})),
            ("algorithm", type("PPOHip", (PPO,), {})), ("algorithm", type("IMPALAOptHip", (IMPALAOpt,), {}))]


def error_name(fn):
    try:
        fn()
    except Exception as exc:      # noqa: BLE001 -- the exception TYPE is what is recorded
        return type(exc).__name__
    return None


def describe(cls):
    return {"name": cls.__name__, "bases": ["{}.{}".format(b.__module__, b.__name__) for b in cls.__bases__]}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference_registry(sys.argv[1])
    registered = {k: {} for k in KINDS}
    for kind, cls in plugin_subclasses():
        assert getattr(ref.Registers, kind)(cls) is cls               # the decorator hands the class back
        registered[kind][cls.__name__] = describe(getattr(ref.Registers, kind)[cls.__name__])
        assert getattr(ref.Registers, kind)[cls.__name__] is cls
    probe = ref.RegisterStub("probe")
    first, second = type("Twice", (object,), {}), type("Twice", (object,), {})
    probe(first)
    probe(second)
    out = {"registered": registered,
           "keys": {k: sorted(getattr(ref.Registers, k)._dict) for k in KINDS},
           "second_registration_wins": probe["Twice"] is second,
           "non_callable_error": error_name(lambda: probe(42)),
           "unknown_name_error": error_name(lambda: probe["NoSuchPlugin"]),
           "instancing_error": error_name(ref.Registers)}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
