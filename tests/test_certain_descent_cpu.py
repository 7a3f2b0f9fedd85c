"""Plumbing of NTR_TRACE_CERTAIN_DESCENT (no device needed): the tunable is parsed, defaults to 1, does not disturb
NTR_TRACE_CERTAIN_STEPS' three values, and leaves every field of ntr_trace_plan's answer as it was."""
import numpy as np
import pytest

import ntrace_amd as nt

MB = 1 << 20


@pytest.fixture(autouse=True)
def clean_tunables(monkeypatch):
    monkeypatch.delenv("NTR_TRACE_CERTAIN_DESCENT", raising=False)
    monkeypatch.delenv("NTR_TRACE_CERTAIN_STEPS", raising=False)
    nt.set_tunables()
    yield
    nt.set_tunables(NTR_TRACE_CERTAIN_DESCENT=None, NTR_TRACE_CERTAIN_STEPS=None)


def test_default_is_on():
    for any_hit in (False, True):
        assert nt.trace_plan_certain(any_hit)["certainDescent"] is True


@pytest.mark.parametrize("text,want", [("0", False), ("1", True), ("2", True), ("", True), ("junk", False)])
def test_the_tunable_is_parsed(text, want):
    nt.set_tunables(NTR_TRACE_CERTAIN_DESCENT=text)      # (an empty value reads as unset, anything else as atoi reads it: the other tunables' rule)
    for any_hit in (False, True):
        assert nt.trace_plan_certain(any_hit)["certainDescent"] is want
    nt.set_tunables(NTR_TRACE_CERTAIN_DESCENT=None)
    assert nt.trace_plan_certain(True)["certainDescent"] is True


def test_certain_steps_keeps_its_three_values():
    for descent in (None, "0", "1"):
        for steps, want in ((None, (False, True)), ("0", (False, False)), ("1", (False, True)), ("2", (True, True))):
            nt.set_tunables(NTR_TRACE_CERTAIN_DESCENT=descent, NTR_TRACE_CERTAIN_STEPS=steps)
            got = tuple(nt.trace_plan_certain(any_hit)["certainSteps"] for any_hit in (False, True))
            assert got == want, (descent, steps)
            assert nt.trace_plan_certain(True)["certainDescent"] is (descent != "0")


def test_the_plan_does_not_see_it():
    fields = [n for n, _ in nt._capi.TracePlan._fields_]
    assert "certainDescent" not in fields and len(fields) == 34

    def plans():
        out = []
        for kernel in ("fermi_speculative_while_while", "kepler_dynamic_fetch", "tesla_persistent_while_while"):
            for any_hit in (False, True):
                for rays in (1000, MB, 1920 * 1080):
                    p = nt.trace_plan(kernel, rays, any_hit, 17 * MB, 17 * MB, bvh_flags=nt.BVH_ORDERED | nt.BVH_FASTDIV)
                    out.append([getattr(p, n) for n in fields])
        return np.array(out)

    base = plans()
    for text in ("0", "1"):
        nt.set_tunables(NTR_TRACE_CERTAIN_DESCENT=text)
        assert np.array_equal(plans(), base), text


def test_null_argument_is_an_error():
    with pytest.raises(nt.NtrError):
        nt._capi._check(nt.lib().ntr_trace_plan_certain(1, None))
