"""The online step's kernel selection (step_plan, pm_query.hip) through pm.step_plan: host arithmetic, no GPU.

Every expected tuple below is written out from the selection rules (the table in tests/test_gpu_step_forms.py,
DESIGN.md §5), not computed: a change to the selector shows here, on the CPU, as the rows it moved.  The forms are
the "host_path_*" counter names in launch order.
"""
import pytest

from tests.test_gpu_step_forms import CASES

ENGINE, SHARED, DEVICE = 0, 1, 2
G = ("match", "resolve_g", "answer_s")            # the three kernels, nothing special about the shape
P8 = ("match_part8", "resolve_g", "answer_s")


def plan(kind, np_, qn, PH=1024, SS=20, E=8, nsub=None, opts=None, **kw):
    import pacmann_amd as pm
    try:
        for k, v in (opts or {}).items():
            pm.set_option(k, v)
        return pm.step_plan(kind, np_, np_ * qn if nsub is None else nsub, qn, PH, SS, E, **kw)
    finally:
        for k in opts or {}:
            pm.set_option(k, -2)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gpu_cases(case):
    """What each GPU case expects to count is what the selector answers for its geometry."""
    import pacmann_amd as pm
    try:
        for k, v in case.opts.items():
            pm.set_option(k, v)
        got = case.plan()
    finally:
        for k in case.opts:
            pm.set_option(k, -2)
    assert got["forms"] == case.forms and got["nhelp"] == case.nhelp, got


@pytest.mark.parametrize("opts,form", [
    ({"match_resolve": 0, "match_part": 1, "match_part8": 1}, "match_part8"),
    ({"match_resolve": 0, "match_part": 1, "match_part8": 0}, "match_part"),
    ({"match_resolve": 0, "match_part": 0}, "match"),
], ids=["part8", "part", "per_subquery"])
def test_hint_search_paths(opts, form):
    """test_batch_pir_group_hint_search_paths: five clients x four partitions (B = 8), 24 ids per client, PH 1,792."""
    assert plan(SHARED, 20, 6, PH=1792, SS=32, opts=opts)["forms"] == (form, "resolve_g", "answer_s")


# (name, kind, np, qn, keywords of plan(), expected forms, expected fields)
ROWS = [
    # ---- k_step: descriptor in the arguments (nsub <= 112, P <= 32), qn <= 64, PH <= 8,192 ----
    ("fused-qn64", ENGINE, 1, 64, {}, ("step",), {"nhelp": 1, "cblk": 1, "nsplit": 0}),   # (240 - 129) / 64 = 1
    ("unfused-qn65", ENGINE, 1, 65, {}, ("match", "resolve_lds", "answer_s"), {"nhelp": 0, "cblk": 1, "nsplit": 1}),
    ("fused-PH8192", ENGINE, 4, 2, {"PH": 8192}, ("step",), {"nhelp": 3}),
    ("unfused-PH8193", ENGINE, 4, 2, {"PH": 8193}, G, {"cblk": 9}),
    ("fused-nsub112-P32", ENGINE, 32, 4, {"nsub": 112}, ("step",), {"nhelp": 0, "args_valid": 1}),   # 2 * 112 + 32 = 256
    ("unfused-nsub113", ENGINE, 32, 4, {"nsub": 113}, G, {"args_valid": 0}),   # (2 nsub + P = 257 needs nsub > 112)
    ("fused-P32", ENGINE, 32, 2, {}, ("step",), {"nhelp": 1}),
    ("unfused-P33", ENGINE, 33, 2, {}, G, {"args_valid": 0}),
    ("no_fuse", ENGINE, 4, 2, {"no_fuse": True}, G, {"nhelp": 0}),
    ("shared-small", SHARED, 4, 2, {}, G, {"args_valid": 1}),      # a group's step is never fused
    ("device-small", DEVICE, 4, 2, {}, G, {"args_valid": 0}),      # the device loop's descriptor is never in the arguments
    # the helpers: min(3, (240 - 2 nsub - P) / nsub), none where 2 nsub + P >= 240 or E & ~3 > 256
    ("help-grid239", ENGINE, 31, 4, {"nsub": 104}, ("step",), {"nhelp": 0}),
    ("help-grid240", ENGINE, 32, 4, {"nsub": 104}, ("step",), {"nhelp": 0}),
    ("help-1", ENGINE, 30, 3, {"nsub": 70}, ("step",), {"nhelp": 1}),       # (240 - 140 - 30) / 70 = 1
    ("help-0", ENGINE, 31, 3, {"nsub": 70}, ("step",), {"nhelp": 0}),       # 69 / 70
    ("help-3", ENGINE, 20, 3, {"nsub": 44}, ("step",), {"nhelp": 3}),       # 132 / 44
    ("help-2", ENGINE, 21, 3, {"nsub": 44}, ("step",), {"nhelp": 2}),       # 131 / 44
    ("help-E259", ENGINE, 4, 2, {"E": 259}, ("step",), {"nhelp": 3}),       # E & ~3 = 256
    ("help-E260", ENGINE, 4, 2, {"E": 260}, ("step",), {"nhelp": 0}),
    ("no_guess", ENGINE, 4, 2, {"no_guess": True}, ("step",), {"no_guess": 1}),
    ("no_guess-unfused", ENGINE, 4, 2, {"no_guess": True, "no_fuse": True}, G, {"no_guess": 0}),
    # ---- the LDS resolver: qn > 64, PH <= 8,192, qn * ceil(PH / 64) <= 2,048 ----
    ("lds-2048", ENGINE, 2, 128, {}, ("match", "resolve_lds", "answer_s"), {}),   # 128 * 16
    ("g-2064", ENGINE, 2, 129, {}, G, {}),
    # ---- the hint search of the three-kernel chain ----
    ("np63", SHARED, 63, 2, {}, G, {}),
    ("np64", SHARED, 64, 2, {}, P8, {}),
    ("np64-nsub127", SHARED, 64, 2, {"nsub": 127}, G, {}),
    ("np64-not-ph8", SHARED, 64, 2, {"ph8": False}, G, {}),
    # ---- k_match_resolve*: shared steps, np >= 128, nsub >= 4 np, words <= 256 ----
    ("np127", SHARED, 127, 4, {}, P8, {"qset": 0}),
    ("np128", SHARED, 128, 4, {}, ("mr_s2", "answer_p5"), {"qset": 1, "qw": 24, "np_live": 0, "nsplit": 1}),
    ("np128-nsub511", SHARED, 128, 4, {"nsub": 511}, P8, {"np_live": 128}),   # (so nsub < 512 never reaches the pair answer)
    ("np128-device", DEVICE, 128, 4, {}, ("mr_s2", "answer_p5"), {}),
    ("np128-engine", ENGINE, 128, 4, {}, P8, {}),                    # an engine's device descriptor is a copy
    ("mr-qn64", SHARED, 128, 64, {}, ("mr_s2", "answer_p5"), {}),
    ("mr-qn65", SHARED, 128, 65, {}, ("match_part8", "resolve_lds", "answer_s"), {}),   # 65 * 16 <= 2,048: the LDS resolver
    ("mr-qn65-PH8192", SHARED, 128, 65, {"PH": 8192}, ("mr_general", "answer_s"), {"np_live": 128}),
    ("mr-PH4096", SHARED, 128, 4, {"PH": 4096}, ("mr_s2", "answer_p5"), {}),
    ("mr-PH4097", SHARED, 128, 4, {"PH": 4097}, ("mr_s4", "answer_p5"), {}),   # (the bound alone: ph8 left set)
    ("mr-PH8192", SHARED, 128, 4, {"PH": 8192}, ("mr_s4", "answer_p5"), {}),
    ("mr-PH8193", SHARED, 128, 4, {"PH": 8193}, ("mr_general", "answer_s"), {"qset": 0}),
    ("mr-not-ph8", SHARED, 128, 4, {"ph8": False}, ("mr_general", "answer_s"), {}),
    ("mr-words256", SHARED, 128, 4, {"PH": 16384}, ("mr_general", "answer_s"), {}),
    ("mr-words257", SHARED, 128, 4, {"PH": 16448}, P8, {"cblk": 17}),
    # ---- the split gather: SetSize >= 256, min(ceil(SS / 48), ceil(4,096 / nsub)) ranges ----
    ("SS255", ENGINE, 2, 16, {"SS": 255, "no_fuse": True}, G, {"nsplit": 1}),
    ("SS256", ENGINE, 2, 16, {"SS": 256, "no_fuse": True}, ("match", "resolve_g", "gather", "answer_g"), {"nsplit": 6}),
    ("SS256-no_split", ENGINE, 2, 16, {"SS": 256, "no_fuse": True, "no_split": True}, G, {"nsplit": 1}),
    ("mr-gather", SHARED, 128, 4, {"SS": 256}, ("mr_s2", "gather", "answer_g"), {"nsplit": 6, "qset": 0, "np_live": 0}),
    # ---- the answer ----
    ("SS1024", ENGINE, 2, 16, {"SS": 1024, "no_fuse": True, "no_split": True}, G, {}),
    ("SS1025", ENGINE, 2, 16, {"SS": 1025, "no_fuse": True, "no_split": True}, ("match", "resolve_g", "answer_g"), {}),
    ("mr-SS1024", SHARED, 128, 4, {"SS": 1024, "no_split": True}, ("mr_s2", "answer_p5"), {"qset": 1, "qw": 1024}),
    ("mr-SS1025", SHARED, 128, 4, {"SS": 1025, "no_split": True}, ("mr_s2", "answer_g"), {"qset": 0, "qw": 0}),
    ("E256", ENGINE, 4, 4, {"E": 256, "no_fuse": True}, G, {}),
    ("E257", ENGINE, 4, 4, {"E": 257, "no_fuse": True}, ("match", "resolve_g", "answer_g"), {}),
    ("pair-E80", SHARED, 128, 4, {"E": 80}, ("mr_s2", "answer_p5"), {}),
    ("pair-E82", SHARED, 128, 4, {"E": 82}, ("mr_s2", "answer_p"), {}),
    ("pair-E9", SHARED, 128, 4, {"E": 9}, ("mr_s2", "answer_s"), {"qset": 1}),   # odd E: no pair form
    ("pair-E256", SHARED, 128, 4, {"E": 256}, ("mr_s2", "answer_p"), {}),
    ("pair-E257", SHARED, 128, 4, {"E": 257}, ("mr_s2", "answer_g"), {}),
    ("pair-E258", SHARED, 128, 4, {"E": 258}, ("mr_s2", "answer_g"), {}),
    # ---- one row per option override ----
    ("opt-match_part1", ENGINE, 4, 2, {"no_fuse": True, "opts": {"match_part": 1}}, P8, {}),
    ("opt-match_part0", SHARED, 128, 4, {"opts": {"match_part": 0, "match_resolve": 0}}, G, {}),
    ("opt-match_part8-0", SHARED, 128, 4, {"opts": {"match_part8": 0, "match_resolve": 0}},
     ("match_part", "resolve_g", "answer_s"), {}),
    ("opt-match_part8-0-nsub511", SHARED, 128, 4, {"nsub": 511, "opts": {"match_part8": 0, "match_resolve": 0}}, G, {}),
    ("opt-match_resolve0", SHARED, 128, 4, {"opts": {"match_resolve": 0}}, P8, {"np_live": 128}),
    ("opt-match_resolve1", SHARED, 128, 4, {"opts": {"match_resolve": 1}}, ("mr_s2", "answer_p5"), {"np_live": 0}),
    ("opt-match_resolve2", SHARED, 128, 4, {"opts": {"match_resolve": 2}}, ("mr_general", "answer_s"), {"np_live": 128}),
    ("opt-answer_waves5", SHARED, 128, 4, {"E": 100, "opts": {"answer_waves": 5}}, ("mr_s2", "answer_p5"), {}),
    ("opt-answer_waves6", SHARED, 128, 4, {"opts": {"answer_waves": 6}}, ("mr_s2", "answer_p"), {}),
    # "step_help" over PM_STEP_HELP: fewer helpers than the budget's 3 (27 fit), never more than the budget's
    ("opt-step_help0", ENGINE, 4, 2, {"opts": {"step_help": 0}}, ("step",), {"nhelp": 0}),
    ("opt-step_help2", ENGINE, 4, 2, {"opts": {"step_help": 2}}, ("step",), {"nhelp": 2}),
    ("opt-step_help3", ENGINE, 4, 2, {"opts": {"step_help": 3}}, ("step",), {"nhelp": 3}),
    ("opt-step_help3-budget1", ENGINE, 32, 2, {"PH": 256, "SS": 8, "opts": {"step_help": 3}}, ("step",), {"nhelp": 1}),   # step-nhelp1
    ("opt-step_help2-E260", ENGINE, 4, 2, {"E": 260, "opts": {"step_help": 2}}, ("step",), {"nhelp": 0}),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_boundaries(row):
    _, kind, np_, qn, kw, forms, fields = row
    got = plan(kind, np_, qn, **kw)
    assert got["forms"] == forms, got
    assert {k: got[k] for k in fields} == fields, got


def test_grids():
    """(counter, grid x, grid y, block) of every launch, one shape per kernel family."""
    assert plan(ENGINE, 4, 2)["launches"] == {"fused": ("step", 2 * 8 + 4 + 3 * 8, 1, 1024)}
    assert plan(ENGINE, 2, 16, PH=8192, SS=296, E=4, no_fuse=True)["launches"] == {
        "match": ("match", 8, 32, 256), "resolve": ("resolve_g", 2, 1, 512),
        "gather": ("gather", 7, 32, 256), "answer": ("answer_g", 32, 1, 512)}
    assert plan(ENGINE, 2, 65, PH=1792)["launches"] == {
        "match": ("match", 2, 130, 256), "resolve": ("resolve_lds", 2, 1, 256), "answer": ("answer_s", 130, 1, 128)}
    assert plan(SHARED, 64, 2, PH=5120)["launches"]["match"] == ("match_part8", 2, 64, 256)   # ceil(5 blocks / 4 waves)
    assert plan(SHARED, 128, 4, PH=5120, opts={"match_part8": 0, "match_resolve": 0})["launches"]["match"] == \
        ("match_part", 5, 128, 256)
    assert plan(SHARED, 129, 5, PH=7168, SS=68, E=4, opts={"answer_waves": 6})["launches"] == {
        "match_resolve": ("mr_s4", 129, 1, 256), "answer": ("answer_p", 323, 1, 128)}   # 645 sub-queries in pairs
    assert plan(SHARED, 128, 4, PH=16384)["launches"]["match_resolve"] == ("mr_general", 128, 1, 512)


@pytest.mark.parametrize("shape", [(ENGINE, 4, 2, {}), (ENGINE, 32, 2, {"PH": 256, "SS": 8}), (ENGINE, 28, 4, {}),
                                   (SHARED, 128, 4, {}), (ENGINE, 2, 65, {"PH": 1792})],
                         ids=["nhelp3", "nhelp1", "nhelp0", "shared", "unfused"])
def test_spoil_changes_no_plan(shape):
    """ "step_help_spoil" (a helper's guess no answer accepts) changes no form, grid or field of any plan."""
    kind, np_, qn, kw = shape
    want = plan(kind, np_, qn, **kw)
    for mask in (1, 2, 4, 7):
        assert plan(kind, np_, qn, opts={"step_help_spoil": mask}, **kw) == want, mask
        assert plan(kind, np_, qn, opts={"step_help_spoil": mask, "step_help": 2}, **kw) == \
            plan(kind, np_, qn, opts={"step_help": 2}, **kw), mask
    assert plan(kind, np_, qn, **kw) == want   # -2 restored both


def test_step_help_option_values():
    import pacmann_amd as pm
    for name, bad, text in (("step_help", (-1, 4), "step_help takes 0..3 or -2"),
                            ("step_help_spoil", (-1, 8), "step_help_spoil takes a mask 0..7 or -2")):
        for v in bad:
            with pytest.raises(RuntimeError, match=text):
                pm.set_option(name, v)
        pm.set_option(name, -2)


def test_rejects():
    import pacmann_amd as pm
    for bad in ((3, 4, 8), (0, 0, 8), (0, 4, 0)):
        with pytest.raises(RuntimeError, match="bad step shape"):
            pm.step_plan(bad[0], bad[1], bad[2], 2, 1024, 20, 8)
