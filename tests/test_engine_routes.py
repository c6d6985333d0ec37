"""ConvEngine's launch routes, pinned without a GPU: the launches and profiling-hook events of every (engine setting, layer) case of
tests/golden/make_golden_engine_routes.py against the recorded table (tests/golden/engine_routes.json)."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_engine_routes", os.path.join(HERE, "golden", "make_golden_engine_routes.py"))
routes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(routes)

EXPECTED = json.load(open(routes.FIXTURE))
CASES = routes.layer_cases()


@pytest.fixture(autouse=True)
def _cpu_stand_ins():
    with routes.cpu_stand_ins():
        yield


def test_fixture_covers_the_grid():
    assert sorted(EXPECTED["cases"]) == sorted(f"{s}/{c}" for s in routes.SETTINGS for c in CASES)


@pytest.mark.parametrize("setting", list(routes.SETTINGS))
def test_routes_match_the_recorded_table(setting):
    for name, case in CASES.items():
        got, _ = routes.run_case(setting, case)
        route, queries = EXPECTED["cases"][f"{setting}/{name}"]
        assert got["events"] == EXPECTED["routes"][route], f"{setting}/{name}"
        assert got["queries"] <= queries, f"{setting}/{name}: {got['queries']} policy queries, {queries} before"


def test_hook_sees_the_same_launch_on_begin_and_end():
    for setting in routes.SETTINGS:
        for name, case in CASES.items():
            _, pairs = routes.run_case(setting, case)
            assert all(len(p) == 2 and p[0] == p[1] for p in pairs), f"{setting}/{name}: has_res on begin / end {pairs}"


def test_dual_refuses_a_layer_marked_acc64():
    """conv_dual has no fp64 form: a layer marked acc64 fails loudly instead of running in fp32 (and nothing is launched)."""
    _, a = CASES["dual"]
    a = dict(a, pc=routes._pc(64 + 256, 256, acc64=True))
    rec, _ = routes.run_case("default", ("dual", a))
    assert rec["events"] == [["raises", "ValueError"]]
    rec, _ = routes.run_case("bf16x3", ("dual", a))            # (acc64 is an fp32-mode promise: bf16x3 runs the fused layer)
    assert [e[0] for e in rec["events"]] == ["begin", "launch", "end"]
