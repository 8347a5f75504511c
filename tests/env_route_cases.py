"""The case table of the env_step route tests, shared by test_env_step_plan_cpu.py (every case plans
as the table says: evx_env_step_plan_query at 256 compute units on dummy pointers) and
test_env_routes_gpu.py (every case steps bit for bit with the oracle on the route it names).

A case is a layout size (L x W interior, R robots, P persons), E envs, the steps to run, the check
interval (every step compares reward and done; every `every` steps the whole state) and flags:

  layouts  0: one layout; n: a LayoutSet of n layouts of this size, env i on layout (7 * i) % n
  nwb      EVX_ENV_NWB for the run (None: unset, the launcher's default)
  jump     the step after which every env's current_step is set to 1190 (None: never): the 1200-step
           time limit then ends every episode about ten steps later
  reset    "fused" (auto_reset=True, obs_term compared on done) or "mask" (env.reset(mask=done))
  wide     compute_order(force=True) before every step: envs with >= hmin persons in play run
           their rows phase on a whole workgroup (rows_wide)
  parts    the wide step as two launches, part 1 then part 2, on one stream
  thmap    the heat map is kept and compared
  floor    None: evacx.layout.synthetic(L, W, R); an integer: random_layout(L, W, R, seed)
  need     the coverage conditions the oracle's own states must meet (env_route_util.run_case):
           "evac", "death", "end" (an episode ended), "near" (a person in play within the repel
           range of a robot at a checked step)
  heavy    wide cases: order[E] is compared with the oracle's count of heavy envs (off where the
           plan has no heavy path and order[E] may be anything)

and the plan the case must get at 256 compute units: env_step_kernel<nwb, multi, bigg>, the
heavy-env cap, and the three LDS layout flags of evx_env_step_plan. The instantiation is part of the
case's name (nwb2-multi-bigg = env_step_kernel<2, true, true>).

The shapes sit on the launcher's and the LDS layout's branches (csrc/env_step.hip: step_plan,
wave_lds, wide_lds, big_grid), with G = (L + 2)(W + 2) cells and bitmaps of RW = ceil(G / 32) words:
the vacated-cell bitmap overlays the Python MT ring while RW <= 624; a grid is big when RW > 1024;
the near-robot block map (one bit per 4 x 4 cells) overlays the shuffle-group region while it has
at most 144 words, which ends at 267 x 267; the 4-wave workgroup must fit 160 KiB of LDS."""
from collections import namedtuple

EnvCase = namedtuple("EnvCase", "name L W R P E steps every flags plan")

HCAP = 176  # heavy_cap's default
PLAN_FIELDS = ("nwb", "bigg", "multi", "hcap", "hmin", "vac_in_ring", "near_in_misc", "wide_past_envs")
FLAG_DEFAULTS = dict(layouts=0, nwb=None, jump=None, reset="fused", wide=False, parts=False, thmap=False, floor=None,
                     need=("evac", "death"), heavy=None)


def instantiation(plan):
    return "nwb%d" % plan["nwb"] + ("-multi" if plan["multi"] else "") + ("-bigg" if plan["bigg"] else "")


def _case(stem, L, W, R, P, E, steps, every, *, nwb_plan, bigg=0, hcap=HCAP, vac=1, near=1, past=0, **flags):
    """nwb_plan, bigg, hcap, vac, near, past: the expected plan (multi follows from layouts)"""
    f = dict(FLAG_DEFAULTS, **flags)
    assert set(f) == set(FLAG_DEFAULTS), sorted(set(f) - set(FLAG_DEFAULTS))
    if f["heavy"] is None:
        f["heavy"] = bool(f["wide"]) and hcap > 0
    if f["jump"] is not None and "end" not in f["need"]:
        f["need"] = tuple(f["need"]) + ("end",)
    plan = dict(nwb=nwb_plan, bigg=bigg, multi=int(f["layouts"] > 0), hcap=hcap,
                hmin=max(1, P // 4) if nwb_plan == 4 else 0, vac_in_ring=vac, near_in_misc=near, wide_past_envs=past)
    name = "%s-%s%s" % (stem, instantiation(plan), "-wide" if f["wide"] and not stem.startswith("wide") else "")
    return EnvCase(name, L, W, R, P, E, steps, every, f, plan)


def _plain_and_wide(stem, *a, **kw):
    """the case with the identity order and again with the forced heavy-first order"""
    return [_case(stem, *a, **kw), _case(stem, *a, wide=True, **kw)]


# ------------------------------------------------------------------ a. kernel variants
# 24x20 / R 4 / P 380 / E 9: 9 % 4 and 9 % 2 leave a partly filled last workgroup
SMALL = (24, 20, 4, 380, 9, 40, 1)
VARIANTS = [_case("small", *SMALL, nwb=n, nwb_plan=n, hcap=HCAP if n == 4 else 0, layouts=k, jump=8)
            for k in (0, 3) for n in (1, 2, 4)]
VARIANTS += [_case("small-maskreset", *SMALL, nwb=4, nwb_plan=4, layouts=k, jump=8, reset="mask") for k in (0, 3)]
# 180x180 (RW 1036): a big grid. 35 steps: the episodes the jump ends at step 15 wipe the counters, and
# the oracle's first death after that comes at step 32
BIG = (180, 180, 2, 3000, 3, 35, 5)
VARIANTS += [_case("big", *BIG, nwb=n, nwb_plan=n, bigg=1, hcap=0, vac=0, layouts=k, jump=5)
             for k in (0, 2) for n in (1, 2)]
# rows_wide on a LayoutSet, in one launch and in two
VARIANTS += [_case("wide", *SMALL, nwb_plan=4, layouts=3, jump=8, wide=True),
             _case("wide-parts", *SMALL, nwb_plan=4, layouts=3, jump=8, wide=True, parts=True)]

# ------------------------------------------------------------------ b. layout boundaries
# pairs: (the two stems, the plan fields in which the two plans differ -- the flag the pair is about,
# and for the big-grid switch what follows from it: two envs per workgroup and no heavy path)
# steps: the oracle's first death comes at step 26 on both sides of the big-grid switch and at steps
# 20 / 33 on the two near-map grids
# Durations (MI355X, one run with test_env_residency_gpu.py, whose slowest case took 0.77 s): the two
# near-map cases take 1.4 s each and big-nwb1-multi-bigg 1.3 s. That time is the host building the
# layout tables (181 fire steps of a 267x267 grid; two 180x180 layouts, shared by the case after it),
# not the stepping (0.03-0.06 s of oracle, less on the device), so fewer steps or envs would not
# shorten them, and their step counts are the fewest that reach the oracle's first death.
VAC = (3, 2500, 2, 30, 5)
BIGSW = (2, 3000, 2, 30, 5)
NEAR = (16, 3000, 2, 35, 5)
BOUNDARIES = (
    _plain_and_wide("vac-126x154", 126, 154, *VAC, nwb_plan=4, vac=1, past=1)       # G 19968, RW 624
    + _plain_and_wide("vac-106x183", 106, 183, *VAC, nwb_plan=4, vac=0, past=1)     # G 19980, RW 625
    + _plain_and_wide("bigsw-179x179", 179, 179, *BIGSW, nwb_plan=4, vac=0, past=1)  # RW 1024: bitmaps in LDS
    + [_case("bigsw-158x203", 158, 203, *BIGSW, nwb_plan=2, bigg=1, hcap=0, vac=0),   # G 32800, RW 1025
       _case("near-266x266", 266, 266, *NEAR, nwb_plan=2, bigg=1, hcap=0, vac=0, near=1,
             need=("evac", "death", "near")),                                        # 67 x 67 blocks: 141 words
       _case("near-267x267", 267, 267, *NEAR, nwb_plan=2, bigg=1, hcap=0, vac=0, near=0,
             need=("evac", "death", "near")),                                        # 68 x 68 blocks: 145 words
       # the 4-wave workgroup exceeds 160 KiB: two envs per workgroup, no heavy path (order[E] free)
       _case("fallback-150x150", 150, 150, 2, 8000, 2, 12, 5, nwb_plan=2, hcap=0, vac=0, past=1, wide=True)]
    # dense crowds: on the steps everybody plans, execute_move sees more order-sensitive occupancy
    # events (a winner's old cell is another mover's target, or its target was vacated by a winner)
    # than its 256-entry LDS list holds (the fallback case above as well, from its step 4 on): the
    # one-wave path, the heavy path's wave 0 and the big-grid path
    + _plain_and_wide("dense-150x150", 150, 150, 2, 6000, 2, 12, 4, nwb_plan=4, vac=0, past=1)
    + [_case("dense-180x180", 180, 180, 2, 12000, 2, 12, 4, nwb_plan=2, bigg=1, hcap=0, vac=0)]
    + _plain_and_wide("aspect-4x300", 4, 300, 2, 100, 4, 40, 1, nwb_plan=4, jump=10)
    + _plain_and_wide("aspect-300x4", 300, 4, 2, 100, 4, 40, 1, nwb_plan=4, jump=10))
BOUNDARY_PAIRS = [
    ("vac-126x154", "vac-106x183", {"vac_in_ring"}),
    ("bigsw-179x179", "bigsw-158x203", {"bigg", "nwb", "hcap", "hmin", "wide_past_envs"}),
    ("near-266x266", "near-267x267", {"near_in_misc"}),
]

# ------------------------------------------------------------------ c. people and robot counts
# tiny grids end episodes by themselves (every person out or dead): "end" without a jump; 4x4 with
# one person never evacuates in 60 steps
_N = ("evac", "death", "end")
COUNTS = []
for (L, W, R, P, need) in [(4, 4, 1, 1, ("death", "end")), (4, 4, 1, 8, _N), (6, 6, 1, 20, _N), (8, 8, 2, 40, _N),
                           (12, 7, 5, 63, _N + ("near",)), (12, 12, 3, 64, _N + ("near",)),
                           (12, 12, 7, 65, _N + ("near",))]:
    COUNTS += _plain_and_wide("people-%dx%d-r%d-p%d" % (L, W, R, P), L, W, R, P, 8, 60, 1, nwb_plan=4, need=need)
for (L, W, R, P) in [(40, 40, 33, 300), (40, 40, 65, 300), (20, 20, 130, 100)]:
    COUNTS += _plain_and_wide("robots-%dx%d-r%d" % (L, W, R), L, W, R, P, 8, 30, 1, nwb_plan=4, jump=10,
                              need=("evac", "death", "near"))
for seed in (11, 12):
    COUNTS += _plain_and_wide("floor-seed%d" % seed, 24, 20, 4, 380, 8, 60, 1, nwb_plan=4, floor=seed, thmap=True,
                              jump=20)

CASES = VARIANTS + BOUNDARIES + COUNTS
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# all ten instantiations of env_step_kernel are named
INSTANTIATIONS = sorted({instantiation(c.plan) for c in CASES})
