"""CPU: the table of tests/mfma_unit_cases.py covers exactly what the build compiles, its dispatch mirror follows the
dispatch sources, and every case is well posed on the restatements alone (the conditions of mfma_unit_cases.failures)."""
import os
import re

import numpy as np
import pytest

import mfma_unit_cases as U
from rlcontrol_amd import build

CASES = U.unit_cases()          # what this tree compiles
TABLE = U.all_cases()           # the whole table: its own conditions hold whatever the build
CSRC = build.CSRC


def _of(family, pred=lambda c: True):
    return [c for c in TABLE if c.NAME == family and pred(c)]


def _widths(c):
    return c.dims[2:]


# ------------------------------------------------------------------------------------------ coverage equals the build
def test_every_compiled_unit_has_a_case_or_a_recorded_refusal():
    compiled = U.compiled_units()
    reached = set(U.unit_of(c) for c in CASES)
    assert reached <= compiled, sorted(reached - compiled)
    assert build.FAST or len(CASES) == len(TABLE)
    assert not (reached & set(U.UNREACHABLE)), sorted(reached & set(U.UNREACHABLE))
    assert reached | set(U.UNREACHABLE) == compiled, sorted(compiled - reached - set(U.UNREACHABLE))
    if not build.FAST:
        assert len(compiled) == 162 + 6
    # a unit kept off the GPU is a compiled unit with a case, named with its reason; the GPU file runs all the others
    assert set(U.NOT_LAUNCHED) <= set(U.unit_of(c) for c in TABLE) and all(U.NOT_LAUNCHED.values())
    assert set(U.unit_of(c) for c in U.gpu_cases()) == reached - set(U.NOT_LAUNCHED)
    print("%d compiled units, %d reached by %d cases, %d unreachable" % (len(compiled), len(reached), len(CASES), len(U.UNREACHABLE)))


def test_case_ids_are_unique_and_name_their_unit():
    ids = [U.case_id(c) for c in TABLE]
    assert len(set(ids)) == len(ids)
    for c, i in zip(TABLE, ids):
        assert i.startswith(U.unit_of(c) + "-") and c.kernel == "mfma"


def test_shapes_are_the_smallest_that_reach_their_unit():
    for c in TABLE:
        wide = U.is_wide(c.S, c.A)
        if c.NAME == "kl":
            assert c.S + c.A <= 8 and (c.kw.get("n_param") == 9 if c.A == 1 else c.kw.get("l_param") in (4, 5)), c.id
            continue
        if "_w_" in U.unit_of(c):
            assert wide and (c.S in (9, 32)) != (c.A >= 3), c.id          # exactly one limit crossed
        else:
            assert not wide, c.id
        assert 200 not in _widths(c), c.id
        if c.NAME in ("sac", "naf") and U.ntw_for(_widths(c)) == 2:
            assert sum(w > U.NTW_SWITCH for w in _widths(c)) == 1 and sorted(_widths(c))[-2] <= 64, c.id
    for fam in ("ddpg", "sac", "naf"):
        wide = _of(fam, lambda c: U.is_wide(c.S, c.A))
        assert set(c.A for c in wide) == set(U.WIDE_ACTION_DIMS) and any(c.S == 32 for c in wide), fam


def test_hidden_widths_cover_every_residue_and_the_extremes():
    full = {0, 4, 8, 12}
    for fam in ("ddpg", "sac", "naf"):
        cases = _of(fam)
        if fam == "ddpg":
            assert set(w % 16 for c in cases for w in _widths(c)) == full
            assert any(len(set(w % 16 for w in _widths(c))) == 3 for c in cases)     # three widths, three residues
        else:
            one = [c for c in cases if U.ntw_for(_widths(c)) == 1]
            two = [c for c in cases if U.ntw_for(_widths(c)) == 2]
            assert set(w % 16 for c in one for w in _widths(c)) == full, fam
            assert set(max(_widths(c)) % 16 for c in two) == full, fam               # the width that decides NTW = 2
        assert {16, 128, 132, 256} <= set(w for c in cases for w in _widths(c)), fam
    sac = _of("sac")
    assert any(max(c.dims[2:4]) <= 128 < max(c.dims[4:6]) for c in sac)              # the actor runs in a unit sized for the critic
    assert any(max(c.dims[4:6]) <= 128 < max(c.dims[2:4]) for c in sac)              # ... and the other way round


def test_batch_sizes_sit_on_both_ends_of_every_tile_count():
    ends = {2: {1, 32}, 4: {33, 64}, 7: {65, 96, 101, 112}, 8: {113, 128}}
    for fam in ("ddpg", "sac", "naf"):
        plain = _of(fam, lambda c: not c.split)
        for mt, want in ends.items():
            got = set(c.B for c in plain if U.mt_for(c.B) == mt)
            assert want <= got, (fam, mt, sorted(want - got))
        assert {97, 100} <= set(c.B for c in plain if U.unit_of(c).endswith("_t4")), fam
    for mt, want in {2: {1, 32}, 7: {33, 112}, 8: {113, 128}}.items():
        assert want <= set(c.B for c in _of("kl") if U.kl_mt_for(c.B) == mt), mt
    split = _of("ddpg", lambda c: c.split)
    assert set(U.unit_of(c) for c in split) == set("ddpg_split_%d_%d" % (m, a) for m in U.SPLIT_MTS for a in (1, 2))
    # ... one of them with a workgroup left without rows at action_dim 2
    assert any(c.A == 2 and U.split_mt(c.B, c.split) * U.SPLIT_ROWS * (c.split - 1) >= c.B for c in split)


def test_kl_cases_reach_all_six_instantiations():
    assert set(U.unit_of(c) for c in _of("kl")) == set(U.KL_UNITS)
    assert set(c.kw["kind"] for c in _of("kl")) == {"reverse", "forward"}


# ------------------------------------------------------------------------------------------ the mirror follows the source
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one_liner(text, signature):
    """the body of a one-line function definition, e.g. 'static inline int mt_for(int B)'"""
    m = re.search(re.escape(signature) + r"\s*\{\s*return\s+(.*?);\s*\}", text)
    assert m, signature
    return m.group(1)


def _ternary_steps(expr):
    """'B <= 32 ? 2 : (B <= 64 ? 4 : 8)' -> ((32, 2), (64, 4), (None, 8))"""
    steps = []
    while True:
        m = re.match(r"\(?\s*B <= (\d+) \? (\d+) : (.*)$", expr.strip())
        if not m:
            last = re.match(r"\(?\s*(\d+)\s*\)*$", expr.strip())
            assert last, expr
            return tuple(steps) + ((None, int(last.group(1))),)
        steps.append((int(m.group(1)), int(m.group(2))))
        expr = m.group(3)


def _macro_lists(text, fast):
    """{name: [tuples]} of the RLC_FOR_* shape lists of one dispatch source, in the branch this build compiles
    (#ifdef RLC_ONLY_7_1 / #else), helper macros with an action_dim parameter expanded"""
    text = text.replace("\\\n", " ")
    defs, branch = {}, []
    for line in text.splitlines():
        s = line.strip()
        if s.startswith("#ifdef RLC_ONLY_7_1"):
            branch.append(True)
        elif s.startswith("#if") :
            branch.append(None)
        elif s.startswith("#else") and branch:
            branch[-1] = None if branch[-1] is None else not branch[-1]
        elif s.startswith("#endif") and branch:
            branch.pop()
        m = re.match(r"#define (RLC_FOR_\w+)\(([^)]*)\)(.*)$", s)
        if m and all(b is None or b == fast for b in branch):
            defs[m.group(1)] = ([p.strip() for p in m.group(2).split(",")], m.group(3))

    def expand(name, args):
        params, body = defs[name]
        out = []
        for call, inner in re.findall(r"(\w+)\(([^()]*)\)", body):
            vals = [dict(zip(params, args)).get(v.strip(), v.strip()) for v in inner.split(",")]
            if call == "X":
                out.append(tuple(int(v) for v in vals))
            else:
                out += expand(call, vals)
        return out
    return {n: expand(n, p) for n, (p, _) in defs.items() if p == ["X"]}


def test_tile_count_thresholds_are_the_sources():
    assert _ternary_steps(_one_liner(_src("ddpg_mfma.hip"), "static inline int mt_for(int B)")) == U.MT_STEPS
    assert _ternary_steps(_one_liner(_src("sac_mfma.hip"), "static inline int sac_mt_for(int B)")) == U.MT_STEPS
    assert _ternary_steps(_one_liner(_src("naf_mfma.hip"), "static inline int naf_mt_for(int B)")) == U.MT_STEPS
    assert _ternary_steps(_one_liner(_src("kl_mfma.hip"), "static inline int kl_mt_for(int B)")) == U.KL_MT_STEPS
    for B in range(1, 129):
        assert U.mt_for(B) == (2 if B <= 32 else 4 if B <= 64 else 7 if B <= 112 else 8)
        assert U.kl_mt_for(B) == (2 if B <= 32 else 7 if B <= 112 else 8)


def test_ntw_switch_is_the_sources():
    naf = _one_liner(_src("naf_mfma.hip"), "static inline int naf_ntw_for(const RlcNafDims& d)")
    assert naf == "(d.L1 <= %d && d.L2 <= %d) ? 1 : 2" % (U.NTW_SWITCH, U.NTW_SWITCH)
    m = re.search(r"static inline int sac_ntw_for\(const RlcSacDims& d\) \{\s*(.*?)\s*\}", _src("sac_mfma.hip"), re.S)
    body = " ".join(m.group(1).split())
    assert body == ("const int w = d.L2A > d.L2C ? d.L2A : d.L2C, k = d.L1A > d.L1C ? d.L1A : d.L1C; "
                    "return (w <= %d && k <= %d) ? 1 : 2;" % (U.NTW_SWITCH, U.NTW_SWITCH))
    assert U.ntw_for((128, 16, 128, 128)) == 1 and U.ntw_for((16, 16, 16, 132)) == 2 and U.ntw_for((132, 16)) == 2


def test_tail_of_four_narrow_wide_and_split_rules_are_the_sources():
    t4 = _one_liner(_src("mfma_blocks.h"), "__host__ __device__ inline bool rlc_tail4(int B, int MT)")
    assert t4 == "B > 16 * (MT - 1) && B <= 16 * (MT - 1) + 4"
    assert [B for B in range(1, 129) if U.tail4(B, U.TAIL4_MT)] == [97, 98, 99, 100]
    assert re.search(r"constexpr int SMAX = %d;" % U.NARROW_S, _src("mfma_blocks.h"))
    assert _one_liner(_src("ddpg_mfma_kernel.h"), "__host__ __device__ inline bool rlc_mfma_wide(const RlcDims& d)") == \
        "d.S > SMAX || d.A > %d" % U.NARROW_A
    for fam, name, dims in (("sac", "rlc_sac_mfma_wide", "RlcSacDims"), ("naf", "rlc_naf_mfma_wide", "RlcNafDims")):
        assert _one_liner(_src(fam + "_common.h"), "inline bool %s(const %s& d)" % (name, dims)) == \
            "d.S > %d || d.A > %d" % (U.NARROW_S, U.NARROW_A)
    m = re.search(r"int rlc_split_mt\(int B, int C\) \{\s*for \(int mt : \{([\d, ]+)\}\)\s*if \(mt \* (\d+) \* C >= B\) return mt;\s*"
                  r"return 0;\s*\}", _src("ddpg_split.hip"))
    assert m and tuple(int(v) for v in m.group(1).split(",")) == U.SPLIT_MTS and int(m.group(2)) == U.SPLIT_ROWS


def test_unit_lists_of_the_dispatch_sources_are_the_compiled_units():
    """a unit added to (or dropped from) a RLC_FOR_* list, or a new kl_launch_t instantiation, fails here and in the
    coverage test until the table is revisited"""
    fast = build.FAST
    d, s, n, sp = (_macro_lists(_src(f), fast) for f in ("ddpg_mfma.hip", "sac_mfma.hip", "naf_mfma.hip", "ddpg_split.hip"))
    names = set("ddpg_mfma_%d_%d" % v for v in d["RLC_FOR_V2"]) | set("ddpg_mfma_%d_%d_t4" % v for v in d["RLC_FOR_T4"])
    names |= set("ddpg_mfma_w_%d_%d" % v for v in d["RLC_FOR_W"]) | set("ddpg_mfma_ln_%d_%d" % v for v in d["RLC_FOR_LN"])
    names |= set("ddpg_split_%d_%d" % v for v in sp["RLC_FOR_SPLIT"])
    for fam, lists in (("sac", s), ("naf", n)):
        up = fam.upper()
        names |= set("%s_mfma_%d_%d_%d" % ((fam,) + v) for v in lists["RLC_FOR_" + up])
        names |= set("%s_mfma_%d_%d_%d_t4" % ((fam,) + v) for v in lists["RLC_FOR_%s_T4" % up])
        names |= set("%s_mfma_w_%d_%d_%d" % ((fam,) + v) for v in lists["RLC_FOR_%s_W" % up])
        assert all(mt == U.TAIL4_MT for mt, _, _ in lists["RLC_FOR_%s_T4" % up])
    assert all(mt == U.TAIL4_MT for mt, _ in d["RLC_FOR_T4"])
    kl = set()
    for f in ("kl_mfma.hip", "kl_mfma_a2.hip"):
        for mt, mtn, ad in re.findall(r"return kl_launch_t<(\d+), (\d+)(?:, (\d+))?>\(", _src(f)):
            assert U.KL_NODE_TILES[int(mt)] == int(mtn)
            kl.add("kl_mfma_%d_%d" % (int(mt), int(ad or 1)))
    assert kl == set(U.KL_UNITS)
    assert names | kl == U.compiled_units(), sorted((names | kl) ^ U.compiled_units())


def test_the_mirror_walks_every_branch():
    assert U.unit_for("ddpg", (3, 1, 200, 200, 200), 100) == "ddpg_mfma_7_1_t4"
    assert U.unit_for("ddpg", (3, 1, 200, 200, 200), 100, split=4) == "ddpg_split_2_1"
    assert U.unit_for("ddpg", (3, 1, 200, 200, 200), 100, sep=True) == "ddpg_mfma_7_1_t4"
    assert U.unit_for("ddpg", (8, 2, 64, 64, 64), 18, norm=True) == "ddpg_mfma_ln_2_2"
    assert U.unit_for("ddpg", (9, 2, 64, 64, 64), 100) == "ddpg_mfma_w_7_2"
    assert U.unit_for("sac", (17, 6, 200, 160, 144, 176), 32) == "sac_mfma_w_2_2_6"
    assert U.unit_for("sac", (3, 2, 128, 96, 112, 128), 100) == "sac_mfma_7_1_2_t4"
    assert U.unit_for("naf", (11, 3, 128, 128), 113) == "naf_mfma_w_8_1_3"
    assert U.unit_for("naf", (8, 2, 200, 200), 101) == "naf_mfma_7_2_2"
    assert U.unit_for("kl", (3, 2, 64, 64, 64, 64), 100) == "kl_mfma_7_2"


# ------------------------------------------------------------------------------------------ well posed on the reference alone
@pytest.mark.parametrize("case", CASES, ids=U.case_id)
def test_case_is_well_posed_on_the_restatements(case):
    """the recorded minibatch seed is the first of (1, ..., 8) at which, on the CPU alone: the oracle's own states pass
    checks b, c, d; no hidden pre-activation of the float64 twin sits on a ReLU kink; every gradient tensor an optimizer
    owns is non-zero after the two warm-up updates; and the fp32 oracle keeps half of every bar against its float64
    twin.  At most half of the list may be left out before it (tests/test_clamp_cases.py)."""
    found = U.find_seed(case)
    assert found is not None, [(s, U.failures(case, s)) for s in U.SEED_LIST[:2]]
    assert found == case.seed, (found, [U.failures(case, s) for s in U.SEED_LIST[:U.SEED_LIST.index(found)]])
    assert U.SEED_LIST.index(found) <= len(U.SEED_LIST) // 2


def test_conditions_reject_what_they_are_there_to_reject():
    """all-zero states under a first layer with zero bias put every first pre-activation exactly on the kink (and leave the
    first layer without gradient): the search can say no"""
    case = [c for c in U.all_cases() if c.NAME == "naf"][0]
    real = case.batch

    def on_the_kink(rng):
        b = list(real(rng))
        b[0] = np.zeros_like(b[0])
        return tuple(b)
    theta0 = case.theta0

    def no_bias(seed=2):
        th = theta0(seed)
        off, shp = case.spec().layout["b1"]
        th[off:off + shp[0]] = 0.0
        return th
    case.batch, case.theta0 = on_the_kink, no_bias
    try:
        out = U.failures(case, 1)
    finally:
        del case.batch, case.theta0
    assert any(f.startswith("kink") for f in out) and any(f.startswith("zero") for f in out), out
