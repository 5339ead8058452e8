"""What the suites that replay the rl_*.npz fixtures through compat's policies (test_rl_pipeline, test_rollout_actions) share."""
import torch


def setup(g):
    """compat's env, robot and value-network policy of a fixture `g`: its weights, visibility, occupancy maps and epsilon."""
    import crowdnav_amd.compat as c
    from crowdnav_amd.compat.sarl import default_policy_config
    with_om, visible = bool(int(g['with_om'])), bool(int(g['robot_visible']))
    name = str(g['policy']) if 'policy' in g else 'sarl'
    cfg = c.default_env_config({('robot', 'visible'): 'true' if visible else 'false'})
    env = c.CrowdSim()
    env.configure(cfg)
    robot = c.Robot(cfg, 'robot')
    policy = c.policy_factory[name]()
    overrides = {(name, 'with_om'): 'true' if with_om else 'false'} if name != 'cadrl' else {}
    if 'pairwise' in g and int(g['pairwise']):
        overrides[('lstm_rl', 'with_interaction_module')] = 'true'
    policy.configure(default_policy_config(overrides))
    policy.get_model().load_state_dict({k[len('param_'):]: torch.from_numpy(v) for k, v in g.items()
                                        if k.startswith('param_')})
    robot.set_policy(policy)
    env.set_robot(robot)
    policy.set_device(torch.device('cpu'))
    policy.set_env(env)
    policy.set_epsilon(float(g['epsilon']))
    return c, env, robot, policy
