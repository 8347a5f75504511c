"""env_step on every kernel variant and on both sides of every LDS layout switch, bit for bit against
the C oracle (env_route_cases.py: the table; env_route_util.run_case: the runner).

Every case first asserts that it takes the route it is named for -- the launcher's own plan
(evx_env_step_plan_query, on this device and at 256 compute units) and the workgroup
evx_env_step_occupancy reports -- then compares reward and done on every step and every state
field, both MT streams and the float64 / float32 observations at its check interval, and ends with
its coverage conditions (an evacuation, a death, an episode end, a person within a robot's range,
the heavy count of the forced order), computed from the oracle's states alone.

Reference: envs/people.py:196-314 (People.run), envs/evacuation_env.py:84-172 (_get_state, step)."""
import pytest
import torch

from env_route_cases import BOUNDARIES, COUNTS, INSTANTIATIONS, VARIANTS
from env_route_util import run_case

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ids(cases):
    return [c.name for c in cases]


def test_every_instantiation_is_named():
    """env_step_kernel<NWB, MULTI, BIGG>: the ten variants step_select can pick"""
    assert INSTANTIATIONS == sorted(["nwb1", "nwb2", "nwb4", "nwb1-multi", "nwb2-multi", "nwb4-multi", "nwb1-bigg",
                                     "nwb2-bigg", "nwb1-multi-bigg", "nwb2-multi-bigg"])


@pytest.mark.parametrize("case", VARIANTS, ids=_ids(VARIANTS))
def test_kernel_variant_matches_oracle(case, monkeypatch):
    """Each instantiation by name (EVX_ENV_NWB, one layout or a LayoutSet, a small or a big grid),
    with a partly filled last workgroup, the time limit's done and both reset flavours; rows_wide
    on a LayoutSet in one launch and in two."""
    _need_gpu()
    print(case.name, run_case(case, monkeypatch))


@pytest.mark.parametrize("case", BOUNDARIES, ids=_ids(BOUNDARIES))
def test_layout_boundary_matches_oracle(case, monkeypatch):
    """Both sides of the vacated-bitmap overlay (RW 624 | 625), the big-grid switch (RW 1024 | 1025)
    and the near-robot map's own region (266 | 267), the heavy path's fallback to two-wave
    workgroups, and 4 x 300 / 300 x 4 grids."""
    _need_gpu()
    print(case.name, run_case(case, monkeypatch))


@pytest.mark.parametrize("case", COUNTS, ids=_ids(COUNTS))
def test_people_and_robot_counts_match_oracle(case, monkeypatch):
    """P = 1 .. 65 around the 64-person groups, R = 1 .. 130 around the 4-robot reads and the 64
    lanes, and obstacle-rich random floors with the heat map."""
    _need_gpu()
    print(case.name, run_case(case, monkeypatch))
