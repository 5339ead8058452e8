"""cn_rollout_route / BatchedCrowdSim.rollout_route: which transition kernel a cn_rollout call would launch, asked of the
host without launching anything (`crowdnav_amd.hip`: rollout_route — the one place the route is chosen)."""
import pytest

from support import amd, environ  # noqa: F401  (amd: module fixture)

pytestmark = pytest.mark.gpu


def _engine(amd, B, H=5, **env):
    with environ(**env):
        return amd.BatchedCrowdSim(num_envs=B, num_humans=H, robot_policy=amd.ROBOT_ORCA, robot_visible=1)


def test_headline_shape_takes_the_two_wave_kernel(amd):
    eng = _engine(amd, 4096)
    before = eng.launch_counts()
    assert eng.rollout_route(20) == 'fused_split' and eng.rollout_route(1000) == 'fused_split'
    assert eng.launch_counts() == before  # asked, not launched


def test_switch_forces_the_one_wave_kernel(amd):
    assert _engine(amd, 4096, CROWDNAV_AMD_FUSED_SPLIT=0).rollout_route(20) == 'fused'


def test_more_envs_than_one_round_keep_the_one_wave_kernel(amd):
    # 2 envs per workgroup, at most 8 two-wave workgroups per CU: 256 CUs hold 4096 envs; 32 768 are eight rounds
    assert _engine(amd, 32768).rollout_route(1000) == 'fused'


def test_fused_off_is_the_generic_kernel(amd):
    assert _engine(amd, 4096, CROWDNAV_AMD_FUSED=0).rollout_route(20) == 'generic'


def test_twenty_humans_never_take_a_fused_kernel(amd):
    assert _engine(amd, 64, H=20).rollout_route(60) in ('generic', 'shard')


def test_abi_version_is_unchanged(amd):
    from crowdnav_amd import _lib
    assert _lib.load().cn_abi_version() == 12
