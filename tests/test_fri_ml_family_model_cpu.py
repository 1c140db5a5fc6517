"""CPU: the Python models of the multilinear FRI opening family (tests/_fri_ml_family_model.py behind the public names of
tests/_fri_ml_{points,arity,grouped,batch}_model.py) still produce the openings recorded in tests/golden/fri_ml_model_openings.json, which
tests/golden/make_fri_ml_model_openings.py wrote from the four separate models that the family model replaced.  Here the cases with d <= 4
(48 of the 84 openings), with the library's host Keccak -- checked against the model's -- for the trees and the transcript; the whole grid is checked by running
that script and comparing its output with the file."""
import importlib.util
import json
import os

import __graft_entry__ as G
import _fri_ml_cases as FC

HERE = os.path.dirname(os.path.abspath(__file__))


def generator():
    spec = importlib.util.spec_from_file_location("make_fri_ml_model_openings", os.path.join(HERE, "golden", "make_fri_ml_model_openings.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_models_reproduce_the_recorded_openings():
    gen = generator()
    with open(gen.OUT) as fh:
        recorded = json.load(fh)
    assert len(recorded) == 84 and all(e["verify"] and not e["verify_changed"] for e in recorded)
    want = [e for e in recorded if e["case"][1] <= 4]
    got = gen.entries(max_d=4, hasher=FC.hasher(G.import_package(), True))
    assert len(want) == 48 and [(e["protocol"], e["case"], e["k"]) for e in got] == [(e["protocol"], e["case"], e["k"]) for e in want]
    for g, w in zip(got, want):
        assert g == w, (w["protocol"], w["case"], w["k"])
