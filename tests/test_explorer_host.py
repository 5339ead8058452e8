"""The host-side rules of compat.Explorer that its drivers share, on the CPU and without an engine: which driver a call takes
(_route), lock-step histories -> episodes (episodes_of_histories = episode_ends + danger_sums), episodes -> the eight values _report takes
(episode_statistics)."""
import numpy as np
import pytest

from crowdnav_amd import _lib
from crowdnav_amd.compat.explorer import danger_sums, episode_ends, episode_statistics, episodes_of_histories

N, DANGER, GOAL, COLL, TIMEOUT = _lib.NOTHING, _lib.DANGER, _lib.REACH_GOAL, _lib.COLLISION, _lib.TIMEOUT


def _setup(robot_policy, target_policy=None):
    """env, robot and policies from the compat classes, as test_rl_pipeline._setup builds them; no device, no engine."""
    import crowdnav_amd.compat as c
    from crowdnav_amd.compat.sarl import default_policy_config
    cfg = c.default_env_config({('robot', 'visible'): 'true'})
    env = c.CrowdSim()
    env.configure(cfg)
    robot = c.Robot(cfg, 'robot')

    def make(name):
        policy = c.policy_factory[name]()
        if name != 'orca':
            policy.configure(default_policy_config({}))
            policy.set_env(env)
        return policy
    policy = make(robot_policy)
    robot.set_policy(policy)
    env.set_robot(robot)
    target = policy if target_policy == robot_policy else make(target_policy) if target_policy else None
    return env, robot, c.Explorer(env, robot, 'cpu', None, 0.9, target_policy=target)


class _ForeignEnv(object):
    """An env that is not this package's (the reference's own CrowdSim has these attributes): no engine_config."""
    case_counter = {'train': 0, 'val': 0, 'test': 0}
    case_size = {'train': 100, 'val': 100, 'test': 100}
    case_capacity = {'train': 100, 'val': 100, 'test': 100}
    human_num, train_val_sim, test_sim = 5, 'circle_crossing', 'circle_crossing'


ROUTES = [
    # id, robot policy, target policy, phase, update_memory, imitation_learning, what the row changes, expected route
    (1, 'orca', None, 'test', False, False, None, 'batched'),
    (2, 'orca', None, 'test', False, False, 'k_wraps', 'sequential'),
    (3, 'orca', None, 'test', False, False, 'counter_-1', 'sequential'),
    (4, 'orca', None, 'train', False, False, None, 'batched'),
    (5, 'sarl', 'sarl', 'val', False, False, None, 'batched'),
    (6, 'sarl', 'sarl', 'train', False, False, None, 'sequential'),
    (7, 'sarl', 'sarl', 'train', True, False, None, 'rl'),
    (8, 'sarl', 'sarl', 'train', True, True, None, 'sequential'),
    (9, 'sarl', 'sarl', 'train', True, False, 'policy_env', 'sequential'),
    (10, 'orca', 'sarl', 'train', True, True, None, 'imitation'),
    (11, 'orca', 'sarl', 'train', True, True, 'unicycle', 'sequential'),
    (12, 'orca', 'orca', 'train', True, True, None, 'sequential'),
]


def _row(robot_policy, target_policy, phase, change):
    env, robot, ex = _setup(robot_policy, target_policy)
    k = 3
    if change == 'k_wraps':
        env.case_counter[phase] = env.case_size[phase] - k + 1   # k is one larger than the cases left in the table
    elif change == 'counter_-1':
        env.case_counter[phase] = -1
    elif change == 'policy_env':
        robot.policy.env = object()
    elif change == 'unicycle':
        ex.target_policy.kinematics = 'unicycle'
    return env, robot, ex, k


@pytest.mark.parametrize('row', ROUTES, ids=lambda r: 'row%d' % r[0])
def test_route_table(row):
    _, robot_policy, target_policy, phase, update_memory, imitation_learning, change, want = row
    env, robot, ex, k = _row(robot_policy, target_policy, phase, change)
    assert ex._route(k, phase, update_memory, imitation_learning) == want
    ex.env = _ForeignEnv()   # row 13: the same call on an env without engine_config
    assert ex._route(k, phase, update_memory, imitation_learning) == 'sequential'


def test_route_refuses_replay_states_under_the_mixed_rule():
    """Row 14: a value network, update_memory, and 'mixed' as the phase's rule — in front of every route."""
    for robot_policy, target_policy, imitation_learning in (('sarl', 'sarl', False), ('orca', 'sarl', True)):
        env, robot, ex = _setup(robot_policy, target_policy)
        robot.policy.multiagent_training = True   # (the train / val phases read the env's rule only then: crowd_sim.py:266-267)
        env.train_val_sim = 'mixed'
        with pytest.raises(NotImplementedError, match='replay states under the mixed rule are ragged'):
            ex._route(1, 'train', True, imitation_learning)
        assert ex._route(1, 'train', False, False) in ('batched', 'sequential')   # acting under it is fine


def test_explorer_constructs_without_env_robot_or_device():
    import crowdnav_amd.compat as c
    ex = c.Explorer(None, None, 'cuda:0')
    assert ex.rl.eng is None and ex.rl.config is None and ex.rl.hist is None and ex.td.graph is None and ex.td.engine is None
    assert ex.rl_profile is None and ex.last_batch is None


def test_earlier_names_of_the_moved_state_read_the_same_objects():
    """_td_graph, _td_engine, _rl_engine_cache and _rl_engine(B, humans, rule) are views of Explorer.td / Explorer.rl."""
    import crowdnav_amd.compat as c
    ex = c.Explorer(None, None, 'cpu')
    assert ex._td_graph is None and ex._td_engine is None and ex._rl_engine_cache is None
    ex.td.graph, ex.td.engine = dict(graph=1), dict(eng=2)
    ex.rl.eng, ex.rl._key, ex.rl._space = 'engine', 'key', 'space'
    assert ex._td_graph is ex.td.graph and ex._td_engine is ex.td.engine and ex._rl_engine_cache == ('key', 'engine', 'space')
    ex.update_target_model(__import__('torch').nn.Linear(2, 1))   # a new target: the graph is dropped, the engine is found stale by its own key
    assert ex._td_graph is None
    seen = []
    ex.env, ex.robot, ex.rl.engine = 'env', 'robot', lambda *a: seen.append(a) or 'e'
    assert ex._rl_engine(1, 5, 'circle_crossing') == 'e' and seen == [('env', 'robot', 1, 5, 'circle_crossing')]


# ------------------------------------------------------------------------------------------------ episode statistics
# success, collision, timeout, success with two Danger steps, collision with none
OUTCOME = [GOAL, COLL, TIMEOUT, GOAL, COLL]
RETURNS = [0.5, -0.25, 0.0, 0.375, -0.125]
DANGER_N = [0, 1, 0, 2, 0]
DANGER_SUM = [0.0, 0.0625, 0.0, 0.25, 0.0]


def test_episode_statistics_with_recorded_end_times():
    times = [10.25, 3.5, 25.25, 11.0, 7.75]
    got = episode_statistics(OUTCOME, times, RETURNS, DANGER_N, DANGER_SUM)
    assert got == ([10.25, 11.0], [3.5, 7.75], [25.25], [1, 4], [2], 3, (0.0 + 0.0625 + 0.0 + 0.25 + 0.0) / 3, RETURNS)
    assert isinstance(got[5], int) and got[7] is RETURNS


def test_episode_statistics_with_step_counts_and_a_timeout_time():
    steps, dt = [41, 14, 101, 44, 31], 0.25
    got = episode_statistics(OUTCOME, [n * dt for n in steps], RETURNS, DANGER_N, DANGER_SUM, 25)
    assert got == ([41 * dt, 44 * dt], [14 * dt, 31 * dt], [25], [1, 4], [2], 3, (0.0 + 0.0625 + 0.0 + 0.25 + 0.0) / 3, RETURNS)
    assert got[2][0] is not None and isinstance(got[2][0], int)   # the timeout time as given, not 101 * dt


def test_episode_statistics_without_success_or_danger():
    got = episode_statistics([COLL, TIMEOUT], [1.5, 25.0], [-0.25, 0.0], [0, 0], [0.0, 0.0], 25)
    assert got == ([], [1.5], [25], [0], [1], 0, 0, [-0.25, 0.0])
    assert got[6] == 0 and isinstance(got[6], int)   # avg_min_dist is 0 when nothing was too close
    assert episode_statistics([], [], [], [], []) == ([], [], [], [], [], 0, 0, [])


# ------------------------------------------------------------------------------------------------ histories -> episodes
def test_episodes_of_histories():
    # env 0 ends at step 1 with stale codes behind the end; env 1 ends at step 4; env 2 has a Danger step before its end
    # (step 3) and another Danger code behind it, which must not count
    info = np.array([[GOAL, N, DANGER],
                     [COLL, N, N],
                     [DANGER, N, COLL],
                     [TIMEOUT, TIMEOUT, DANGER]], dtype=np.uint8)
    dmin = np.array([[9.0, 9.0, 0.125],
                     [0.5, 9.0, 9.0],
                     [0.25, 9.0, 9.0],
                     [9.0, 9.0, 0.0625]])
    steps, last, danger_n, danger_sum, keep = episodes_of_histories(info, dmin)
    assert steps.tolist() == [1, 4, 3] and last.tolist() == [GOAL, TIMEOUT, COLL]
    assert danger_n == [0, 0, 1] and danger_sum == [0.0, 0.0, 0.125]
    assert keep.tolist() == [0, 2]   # ReachGoal / Collision episodes enter the memory, the timeout does not
    assert all(type(n) is int for n in danger_n) and all(type(s) is float for s in danger_sum)
    # the two halves the RL driver runs in front of and behind its push
    assert [a.tolist() for a in episode_ends(info)] == [[1, 4, 3], [GOAL, TIMEOUT, COLL], [0, 2]]
    assert danger_sums(info, dmin, steps) == ([0, 0, 1], [0.0, 0.0, 0.125])


def test_episodes_of_histories_needs_an_end_code_from_every_env():
    info = np.array([[GOAL, N, N], [N, DANGER, COLL], [N, N, N], [N, N, TIMEOUT]], dtype=np.uint8)   # env 1 never ends
    with pytest.raises(ValueError, match='Invalid end signal from environment'):
        episodes_of_histories(info, np.zeros((4, 3)))
