"""CPU: the outputs of the two Levenberg-Marquardt loops' host forms (mi355_global_projective_refine*, mi355_calibrate_lens*) and of the
flat list's run splitter, bit for bit against tests/golden/lm_loops_parent.json.  The fixture was recorded from the commit it names, before
the two refinements were folded onto one block skeleton and one loop driver (csrc/tie_blocks.h); the device tests compare device against
host, which change together, so this is what holds both to the bits of that commit.  Per case: the sha1 of the output bytes and the whole
report, floats as repr.  The arithmetic is + - * / and sqrt under -ffp-contract=off, so the bytes do not depend on the machine.

    python -m tests.test_lm_loops_parent COMMIT      records the fixture from the library as built"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import imagemosaicing_amd as im
from tests import calib_cases as cc
from tests import projective_cases as pc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_loops_parent.json")
_SURVEYS = {}


def _entry(out, rep):
    return {"sha1": hashlib.sha1(bytes(out) if not isinstance(out, np.ndarray) else out.tobytes()).hexdigest(), "report": {k: repr(v) for k, v in rep.items()}}


def _survey(name, noise):
    if (name, noise) not in _SURVEYS:
        s = pc.survey(name, noise)
        _SURVEYS[(name, noise)] = (s, im.results_to_match_pairs(s["recs"]))
    return _SURVEYS[(name, noise)]


def long_run_list():
    """strip12's flat list with the ties of pair (0, 1) repeated to a run of more than 400: two blocks for the refinements, one pair for the
    affine alignment"""
    s, flat = _survey("strip12", 0.5)
    first = flat[(flat["ai"] == 0) & (flat["bi"] == 1)]
    reps = 400 // len(first) + 2
    v = np.concatenate([first] * reps + [flat[len(first):]])
    assert 8 <= len(first) and 400 < reps * len(first) < 800 and len(v) == len(flat) + (reps - 1) * len(first)
    return s, v


def projective(name, noise, prior, form):
    s, flat = _survey(name, noise)
    fn, data = (im.global_projective_refine_results, s["recs"]) if form == "results" else (im.global_projective_refine, flat)
    return _entry(*fn(data, s["w"], s["h"], s["start"], params=im.projective_params(prior=prior)))


def calibration(name, noise, mask, form):
    fn, data = (im.calibrate_lens_results, cc.survey(name, noise)) if form == "results" else (im.calibrate_lens, cc.flat_survey(name, noise))
    return _entry(*fn(data, im.Camera(*cc.CAM_START), mask=mask))


def splitter(which):
    s, v = long_run_list()
    if which == "projective":
        return _entry(*im.global_projective_refine(v, s["w"], s["h"], s["start"]))
    if which == "affine":
        return _entry(im.global_affine_align(v, s["n"]), {})
    if which == "records":
        recs = im.match_pairs_to_results(v)
        return _entry(recs, {"records": len(recs), "longest": int(recs["n_in"].max())})
    return _entry(*im.calibrate_lens(v, im.Camera(*cc.CAM_START)))


CASES = ([("projective", n, z, p, f) for n in ("grid16", "strip12") for z in (0.0, 0.5) for p in (0.0, 0.01) for f in ("results", "flat")] +
         [("calibration", n, z, m, f) for n in ("grid16", "strip12") for z in (0.0, 0.5) for m in (3, 31) for f in ("results", "flat")] +
         [("splitter", w) for w in ("projective", "affine", "records", "calibration")])
RUN = {"projective": projective, "calibration": calibration, "splitter": splitter}


def case_id(case):
    return "-".join(str(c) for c in case)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_outputs_equal_the_parent_commit_bits(case, golden):
    got = RUN[case[0]](*case[1:])
    assert got == golden["cases"][case_id(case)]


def test_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden["cases"]) == sorted(case_id(c) for c in CASES) and len(golden["commit"]) == 40
    loops = [e["report"] for k, e in golden["cases"].items() if "trials" in e["report"]]
    assert len(loops) == 34 and all(int(r["accepted"]) >= 1 for r in loops) and any(int(r["trials"]) > int(r["accepted"]) for r in loops)       # both branches of the schedule
    assert golden["cases"]["splitter-records"]["report"]["longest"] == "400"


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump({"commit": sys.argv[1], "cases": {case_id(c): RUN[c[0]](*c[1:]) for c in CASES}}, f, indent=1, sort_keys=True)
        f.write("\n")
