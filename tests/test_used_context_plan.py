"""CPU: the step tables of tests/used_context.py can show a leak.  From the cases' own numbers, without the library: for every shared buffer of
a family some step follows one that left MORE in that buffer than the step itself writes; the two steps run on different cases and their
references differ (a neighbour with the same frame count and the same lists would prove nothing); and every reference a GPU test will use is
computed here once, so that a broken reference fails on the CPU and not first on the GPU machine.
"""
import numpy as np
import pytest

from tests import used_context as uc

FAMILIES = {"renders": (uc.render_steps, uc.RENDER_SHARED), "chips": (uc.chip_steps, uc.CHIP_SHARED), "pairs": (uc.pair_steps, uc.PAIR_SHARED)}
_REFS = {}


def _refs(family, orc):
    """every step's reference, computed once"""
    if family not in _REFS:
        steps = FAMILIES[family][0]()
        _REFS[family] = (steps, [None if s.ref is None else s.ref(orc) for s in steps])
    return _REFS[family]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_reference_is_computable(oracle, family):
    steps, refs = _refs(family, oracle)
    assert len({s.name for s in steps}) == len(steps) >= 10
    for s, r in zip(steps, refs):
        assert r is not None and any(v is not None for v in r), s.name + ": a step without a reference"
        for v in r:
            assert v is None or uc.as_array(v).size > 0, s.name


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_shared_buffer_meets_a_smaller_call_after_a_larger_one(oracle, family):
    steps, refs = _refs(family, oracle)
    make, shared = FAMILIES[family]
    assert set(shared) <= set(uc.buffers_of(steps)), sorted(set(shared) - set(uc.buffers_of(steps)))
    for buffer in shared:
        chances = uc.leak_chances(steps, buffer)
        assert chances, buffer + ": no step follows one that left more there"
        proving = 0
        for i, j in chances:
            left, written = steps[j].leaves[buffer], steps[i].leaves[buffer]
            assert left > written >= 0 and j < i                            # more was left than is written
            if steps[i].case != steps[j].case and uc.references_differ(refs[i], refs[j]):
                proving += 1
        assert proving, buffer + ": every smaller step has the same case or the same reference as the larger one before it"


def test_render_order_puts_the_sharing_renders_next_to_each_other():
    steps = uc.render_steps()
    names = [s.name for s in steps]
    writes_owner = [i for i, s in enumerate(steps) if "seamline_owner" in s.leaves]
    kinds = [names[i].split()[0] for i in writes_owner]
    assert any(a == "seamline" and b == "seamcut" and j == i + 1 for (i, a), (j, b) in zip(zip(writes_owner, kinds), zip(writes_owner[1:], kinds[1:])))
    assert any(a == "seamcut" and b == "seamline" and j == i + 1 for (i, a), (j, b) in zip(zip(writes_owner, kinds), zip(writes_owner[1:], kinds[1:])))
    # a refined step (no ramps, no frame_of) directly before a median and before a seamcut step with fewer frames than the ramps left behind
    for kind in ("median", "seamcut"):
        found = False
        for i in range(1, len(steps)):
            if names[i].startswith(kind) and names[i - 1].startswith("refined") and "feather_ramps" not in steps[i - 1].leaves:
                ramps_behind = max(s.leaves.get("feather_ramps", 0) for s in steps[:i])
                found |= steps[i].leaves["feather_ramps"] < steps[i - 1].leaves["mosaic_frames"] <= ramps_behind
        assert found, kind
    V = uc.render_surveys()
    assert V["L"].blocks() == 4 and V["W"].n == 130 and V["W"].blocks() == 1 and V["S"].n == 2 and (V["B"].cw, V["B"].ch) == (32, 124)
    assert max(max(a.shape[:2]) for S in V.values() for a in S.imgs) <= 160 and max(S.n for S in V.values()) <= 130


def test_the_runner_names_the_step_and_the_first_difference():
    a = [np.zeros((3, 4), np.uint8), dict(x=1, y=2)]
    b = [np.zeros((3, 4), np.uint8), dict(x=1, y=3)]
    assert uc.first_difference(a, a) is None and uc.first_difference(a, [None, None]) is None
    assert uc.first_difference(a, b) == "output 1: 1 of 2 values differ, first at [[1]]"
    b[0][2, 1] = 9
    assert uc.first_difference(a, b) == "output 0: 1 of 12 values differ, first at [[2, 1]]"
    assert "shape" in uc.first_difference(a, [np.zeros((3, 5), np.uint8), a[1]])
    assert uc.references_differ(a, b) and not uc.references_differ(a, a)
