"""CPU: the Python models of the zerocheck family (tests/_zerocheck_family_model.py behind the public names of tests/_zerocheck_model.py,
_zerocheck_gate_model.py, _wiring_model.py, _plonk_model.py, _lookup_model.py, _plonk_lookup_model.py and _plonk_lookup_columns_model.py) still
produce the proofs, verdicts, sizes and C arrays recorded in tests/golden/zerocheck_family_model_proofs.json, which
tests/golden/make_zerocheck_family_model_proofs.py wrote from the seven separate models that the family model replaced.  The whole grid, with
the library's host Keccak -- checked against the model's -- for the trees and the transcript."""
import importlib.util
import json
import os

import __graft_entry__ as G
import _fri_ml_columns_model as CM

HERE = os.path.dirname(os.path.abspath(__file__))
KEY = ("protocol", "case", "schedule", "variant")


def generator():
    spec = importlib.util.spec_from_file_location("make_zerocheck_family_model_proofs", os.path.join(HERE, "golden", "make_zerocheck_family_model_proofs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_generators_cases_are_the_cpu_tests_cases():
    import test_lookup_cpu, test_plonk_cpu, test_plonk_lookup_columns_cpu, test_plonk_lookup_cpu, test_wiring_cpu, test_zerocheck_cpu, test_zerocheck_gate_cpu
    gen = generator()
    mods = (test_zerocheck_cpu, test_zerocheck_gate_cpu, test_wiring_cpu, test_plonk_cpu, test_lookup_cpu, test_plonk_lookup_cpu, test_plonk_lookup_columns_cpu)
    for kind, mod in zip(gen.KINDS, mods):
        assert list(kind.cases) == [c for c in mod.CASES if c[1] <= 4], kind.name
    assert all(m.SCHEDULES == gen.SCHEDULES for m in mods[:-1]) and gen.Q == 4


def test_the_models_reproduce_the_recorded_proofs():
    gen = generator()
    with open(gen.OUT) as fh:
        want = json.load(fh)
    assert len(want) == 466 and all("flat" in e for e in want)
    zk = G.import_package()
    got = json.loads(json.dumps(gen.entries(hasher=CM.check_host_keccak(zk), zk=zk)))
    assert [[e[k] for k in KEY] for e in got] == [[e[k] for k in KEY] for e in want]
    for g, w in zip(got, want):
        assert g == w, [w[k] for k in KEY]
