"""What a context decides about itself, asked without a context or a device (csrc/ctx_params.cpp through bce_params_derive
and bce_dag_launch_choice).

The derivation is held to the commit before it became a function of its own: tests/golden/ctx_params_pins.json was written by
tests/golden/make_ctx_params_pins.py from that commit's build_ctx() and derive_ctx(), on a machine without a GPU, for the
tabulated sets, custom shapes at every edge the code names, every rejected argument and each context knob alone.  Every named
value, table digest, status and message must be equal.

The launch choice of bce_dag_run had no entry a probe could reach; its expectations are worked out by hand from the rule and
written next to each case.
"""
import importlib.util
import os

import pytest

from conftest import GOLDEN

CTX_KNOBS = ["BCE_VARIANT", "BCE_FUSE_TAIL", "BCE_OCCUPANCY", "BCE_FP64", "BCE_XCD_GATE", "BCE_XCD_GATE_US", "BCE_FOLD", "BCE_FWD_UNITS",
             "BCE_FWD_MFMA"]
DAG_KNOBS = ["BCE_DAG_GATE_US", "BCE_DAG_GATE_BACKLOG", "BCE_DAG_WPS", "BCE_DAG_PLACE", "BCE_DAG_DEBUG", "BCE_DAG_GATE", "BCE_DAG_TICKETS"]


def _pins():
    spec = importlib.util.spec_from_file_location("make_ctx_params_pins", os.path.join(GOLDEN, "make_ctx_params_pins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PINS = _pins()
ROWS = PINS.load()


@pytest.fixture
def no_knobs(monkeypatch):
    for k in CTX_KNOBS + DAG_KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _derive(bce, case):
    if "set" in case:
        return bce.derive_params(case["set"][0], case["set"][1], cu_count=case["cu"])
    return bce.derive_params(method=case["custom"][8], cu_count=case["cu"], custom=case["custom"][:8])


def test_the_fixture_covers_what_it_must():
    ids = {r[0] for r in ROWS}
    assert len(ROWS) >= 100 and os.path.getsize(PINS.FIXTURE) < 100 * 1024
    assert {"%s/%s" % (s, m) for s in PINS.SETS for m in PINS.METHODS} <= ids
    assert {"n=%d" % n for n in (887, 888, 895, 896, 2423, 2424, 2431, 2432)} <= ids
    knob_rows = [r for r in ROWS if r[2]]
    assert len(knob_rows) == 3 * 11 and {k for r in knob_rows for k in r[2]} == set(CTX_KNOBS)
    by_id = {r[0]: r for r in ROWS}
    # the shapes the cases were chosen for do what they were chosen for
    assert by_id["MEDIUM/GINX"][5]["lazy"] == 0 and by_id["STD128_OPT/GINX"][5]["lazy"] == 1
    assert by_id["TOY/GINX"][5]["fold"] == 0
    # ... and where a folded build exists, so that the exactness test alone decides (Q / 2 > 511 (1 + 2^10 + 2^20) + 1)
    assert by_id["N=2048,30bit,3digits"][5]["fold_build"] == 1 and by_id["N=2048,30bit,3digits"][5]["fold"] == 0
    assert by_id["odd-factor"][5]["factor_even"] == 0 and by_id["odd-factor"][5]["fwd_units"] == 0
    assert [by_id["n=%d" % n][5]["fwd_mfma"] for n in (895, 896)] == [1, 0]
    assert [by_id["n=%d" % n][5]["wg_per_cu_full"] for n in (2431, 2432)] == [2, 1]
    assert by_id["AP,n=511"][5]["family"] == 1 and by_id["AP,n=512"][5]["family"] == 0       # key of 2^31 bytes: not below it
    assert [by_id["qKS=%d" % v][5]["ksk_u16"] for v in (65536, 65537)] == [1, 0]
    assert by_id["Q<2^28"][5]["is64"] == 0 and by_id["Q>2^28"][5]["is64"] == 1
    assert by_id["Q<2^39/GINX"][5]["fp64"] == 1 and by_id["Q>2^39/GINX"][5]["fp64"] == 0
    assert [(by_id["N=2048,Q<2^39,B=2^%d" % b][5]["fold_build"], by_id["N=2048,Q<2^39,B=2^%d" % b][5]["fold"]) for b in (14, 16)] == [(1, 1), (1, 0)]
    assert {by_id[i][5]["dG"] for i in ("N=1024,3digits", "N=1024,4digits")} == {3, 4}
    assert sum(r[3] != 0 for r in ROWS) >= 25


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_derive_params_equals_the_parent(bce, no_knobs, row):
    cid, case, knobs, status, message, values = row
    for k, v in knobs.items():
        no_knobs.setenv(k, v)
    got = _derive(bce, case)
    assert (got.pop("status"), got.pop("message")) == (status, message)
    if status == 0:
        assert sorted(got) == sorted(values), "the named values differ from the fixture's"
        assert {k: (got[k], values[k]) for k in got if got[k] != values[k]} == {}


def test_unknown_set_and_null_output(bce, no_knobs):
    assert bce.derive_params(99, bce.GINX) == {"status": bce.ERR_ARG, "message": "unknown parameter set"}
    assert bce.derive_params(-1, bce.GINX)["status"] == bce.ERR_ARG
    assert bce.lib().bce_params_derive_set(bce.STD128_OPT, bce.GINX, 256, None, None) == bce.ERR_ARG


def test_names_are_the_enum(bce):
    import re
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "bce_gpu.h")) as f:
        text = f.read()
    for prefix, names in (("BCE_D_", bce.D_NAMES), ("BCE_L_", bce.L_NAMES)):
        enum = re.search(r"enum \{ (%s\w+ = 0,.*?)\};" % prefix, text, re.S).group(1)
        assert re.findall(prefix + r"(\w+)", enum) == names + ["COUNT"]


# ---- launch choice ------------------------------------------------------------------------------------------------------
# The rule (bce_dag_run): wps = 2 (one workgroup per CU) or 4 (two).  workgroups_per_cu 1 / 2 force 2 / 4; 0 compares
# t1 = max(depth, items / cus) with t2 = max(1.6 depth, items / (1.26 cus)) and takes one per CU when t1 <= t2.  Then, in this
# order: BCE_DAG_WPS = 2 / 4; wg_per_cu_full == 1 forces one; two workgroups of the persistent kernel whose LDS exceeds 160 KiB
# force one (32-bit contexts).  grid = cus x workgroups per CU.  policy: bit 0 placement (BCE_DAG_PLACE overrides), bit 1
# BCE_DAG_DEBUG=d, bit 2 the start gate (BCE_DAG_GATE, unset: with two per CU), bit 3 BCE_DAG_TICKETS=1.

def _report(bce, cus=256, is64=0, wg_full=2, dag_lds=70000):
    d = dict.fromkeys(bce.D_NAMES, 0)
    d.update(cu_count=cus, is64=is64, wg_per_cu_full=wg_full, dag_lds_bytes=dag_lds)
    return d


ONE = dict(wps=2, grid=256, policy=1)            # placement only
TWO = dict(wps=4, grid=512, policy=1 | 4)        # placement + gate
DEFAULTS = dict(gate_ticks=15000, gate_backlog=8, lazy_ticks=2000, stall_ticks=400000000, rearm_only=0)
SHALLOW = dict(depth=10, items=100)      # t1 = max(10, 0.39) = 10 <= t2 = max(16, 0.31) = 16: one per CU
WIDE = dict(depth=1, items=100000)       # t1 = max(1, 390.6) = 390.6 > t2 = max(1.6, 310.0) = 310.0: two per CU

CHOICES = [
    ("shallow", {}, SHALLOW, {}, {}, ONE),
    ("wide", {}, WIDE, {}, {}, TWO),
    # t1 == t2 at depth = items / cus exactly?  depth 100, items 25600: t1 = 100, t2 = max(160, 79.4) = 160: one
    ("balanced", {}, dict(depth=100, items=25600), {}, {}, ONE),
    # depth 100, items 51200: t1 = 200, t2 = max(160, 158.7) = 160: two
    ("twice-the-chip", {}, dict(depth=100, items=51200), {}, {}, TWO),
    ("forced-one", {}, WIDE, dict(workgroups_per_cu=1), {}, ONE),
    ("forced-two", {}, SHALLOW, dict(workgroups_per_cu=2), {}, TWO),
    ("lds-holds-one", dict(wg_full=1), WIDE, {}, {}, ONE),
    ("lds-holds-one-forced-two", dict(wg_full=1), WIDE, dict(workgroups_per_cu=2), {}, ONE),
    # 2 x 81920 = 160 KiB exactly fits; one byte more does not; the 64-bit kernels are not measured by this figure
    ("dag-lds-fits", dict(dag_lds=81920), WIDE, {}, {}, TWO),
    ("dag-lds-retreat", dict(dag_lds=81921), WIDE, {}, {}, ONE),
    ("dag-lds-retreat-forced-two", dict(dag_lds=81921), SHALLOW, dict(workgroups_per_cu=2), {}, ONE),
    ("dag-lds-64bit", dict(dag_lds=81921, is64=1), WIDE, {}, {}, TWO),
    ("64-cus", dict(cus=64), dict(depth=1, items=100), {}, {}, dict(wps=2, grid=64, policy=1)),   # t1 = 1.56 <= t2 = 1.6
    ("64-cus-wide", dict(cus=64), dict(depth=1, items=200), {}, {}, dict(wps=4, grid=128, policy=5)),   # t1 = 3.1 > t2 = 2.5
    ("no-cus", dict(cus=0), WIDE, {}, {}, dict(wps=4, grid=0, policy=5)),    # cus counts as 1 in the rule, the grid is what it is
    ("placement-off", {}, SHALLOW, dict(placement=0), {}, dict(ONE, policy=0)),
    ("ticks", {}, SHALLOW, dict(lazy_us=7, stall_ms=40000), {}, dict(ONE, lazy_ticks=700, stall_ticks=4000000000)),
    ("ticks-wrap", {}, SHALLOW, dict(lazy_us=50000000, stall_ms=4000), {}, dict(ONE, lazy_ticks=(50000000 * 100) % 2**32)),
    # each DAG knob alone
    ("GATE_US", {}, WIDE, {}, {"BCE_DAG_GATE_US": "40"}, dict(TWO, gate_ticks=4000)),
    ("GATE_US=0", {}, WIDE, {}, {"BCE_DAG_GATE_US": "0"}, dict(TWO, gate_ticks=0)),
    ("GATE_BACKLOG", {}, WIDE, {}, {"BCE_DAG_GATE_BACKLOG": "64"}, dict(TWO, gate_backlog=64)),
    ("WPS=2", {}, WIDE, {}, {"BCE_DAG_WPS": "2"}, ONE),
    ("WPS=4", {}, SHALLOW, {}, {"BCE_DAG_WPS": "4"}, TWO),
    ("WPS=3", {}, SHALLOW, {}, {"BCE_DAG_WPS": "3"}, ONE),                     # neither: the rule stands
    ("WPS=4-over-forced-one", {}, SHALLOW, dict(workgroups_per_cu=1), {"BCE_DAG_WPS": "4"}, TWO),
    ("WPS=4-loses-to-lds", dict(wg_full=1), SHALLOW, {}, {"BCE_DAG_WPS": "4"}, ONE),
    ("WPS=4-loses-to-dag-lds", dict(dag_lds=81921), SHALLOW, {}, {"BCE_DAG_WPS": "4"}, ONE),
    ("PLACE=0", {}, SHALLOW, {}, {"BCE_DAG_PLACE": "0"}, dict(ONE, policy=0)),
    ("PLACE=1-over-limits", {}, SHALLOW, dict(placement=0), {"BCE_DAG_PLACE": "1"}, dict(ONE, policy=1)),
    ("PLACE-empty", {}, SHALLOW, dict(placement=0), {"BCE_DAG_PLACE": ""}, dict(ONE, policy=1)),   # set, and not '0'
    ("DEBUG=r", {}, SHALLOW, {}, {"BCE_DAG_DEBUG": "r"}, dict(ONE, rearm_only=1)),
    ("DEBUG=d", {}, SHALLOW, {}, {"BCE_DAG_DEBUG": "d"}, dict(ONE, policy=1 | 2)),
    ("GATE=0-against-two", {}, WIDE, {}, {"BCE_DAG_GATE": "0"}, dict(TWO, policy=1)),
    ("GATE=1-against-one", {}, SHALLOW, {}, {"BCE_DAG_GATE": "1"}, dict(ONE, policy=1 | 4)),
    ("GATE-follows-the-final-wps", dict(wg_full=1), WIDE, {}, {}, dict(ONE, policy=1)),
    ("TICKETS=1", {}, WIDE, {}, {"BCE_DAG_TICKETS": "1"}, dict(TWO, policy=1 | 4 | 8)),
    ("TICKETS=0", {}, WIDE, {}, {"BCE_DAG_TICKETS": "0"}, TWO),
]


@pytest.mark.parametrize("name,report,dag,limits,env,expect", CHOICES, ids=[c[0] for c in CHOICES])
def test_dag_launch_choice(bce, no_knobs, name, report, dag, limits, env, expect):
    for k, v in env.items():
        no_knobs.setenv(k, v)
    got = bce.dag_launch_choice(_report(bce, **report), dag["depth"], dag["items"], **limits)
    assert got == dict(DEFAULTS, **expect)


def test_dag_launch_choice_of_a_derived_report(bce, no_knobs):
    """the report of derive_params carries what the choice reads: STD128_OPT / GINX runs the matrix-pipe body, whose
    persistent build fits twice (n = 502); at n = 888 it does not although two workgroups of the per-frontier kernel do"""
    d = bce.derive_params(bce.STD128_OPT, bce.GINX)
    assert d["dag"] == 1 and d["wg_per_cu_full"] == 2 and 0 < 2 * d["dag_lds_bytes"] <= 160 * 1024
    assert bce.dag_launch_choice(d, **WIDE) == dict(DEFAULTS, **TWO)
    by_id = {r[0]: r for r in ROWS}
    for n, two in ((887, True), (888, False), (896, True), (2423, True), (2424, False)):
        d = _derive(bce, by_id["n=%d" % n][1])
        assert d["wg_per_cu_full"] == 2 and (2 * d["dag_lds_bytes"] <= 160 * 1024) == two, n
        assert bce.dag_launch_choice(d, **WIDE)["wps"] == (4 if two else 2), n
