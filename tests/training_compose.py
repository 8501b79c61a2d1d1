"""The two-agent training turn COMPOSED from calls that exist without mcbs_two_agent_train_step — `att.step` (auto-resetting),
`dfd.step`, `engine.reset(mask)`, `engine.observe(obs, mask)`, `dfd.reset(mask)` and tensor assignments into the wrappers' public state —
following the rules of include/mcbs.h.  It is what tests/test_gpu_two_agent_training.py holds the one-launch turn to, bit for bit, and
the baseline leg of tools/bench_two_agent_training.py: the only way to run this loop without the new entry point.  Everything is
enqueued on the device (masked `where` assignments, no host synchronisation), so the timing is the composition's and not a host stall's."""


class ComposedTrainingTurn:
    def __init__(self, att, dfd):
        self.att, self.dfd = att, dfd
        t = self.torch = att.torch
        E, dev = att.num_envs, att.engine.device
        self.request = t.zeros(E, dtype=t.bool, device=dev)
        self.defender_returns = t.zeros(E, dtype=t.float64, device=dev)
        self.terminal = {k: t.zeros_like(v) for k, v in dfd.observation.items()}
        self.mask = None
        self.reset()

    def reset(self):
        self.att.reset()
        self.dfd.reset()
        self.request.zero_()
        self.defender_returns.zero_()

    @staticmethod
    def _rows(mask, like):
        return mask.view((-1,) + (1,) * (like.dim() - 1))

    def step(self, a1, a2, with_mask=True):
        """-> (attacker outputs, defender outputs): dicts of device tensors, the names TwoAgentTrainVecEnv's tuples and infos use"""
        t, att, dfd, eng = self.torch, self.att, self.dfd, self.att.engine
        q = self.request
        v0, i0 = att.valid_action_count.clone(), att.invalid_action_count.clone()
        # ---- attacker half: the auto-resetting wrapper step, then the same reset for the envs that end only because they were asked ----
        _, r1, term1, trunc1, info = att.step(a1)
        own = (term1 | trunc1) != 0
        forced = q & ~own
        invalid = info["invalid_action"]
        a = dict(rewards=r1, terminated=term1, truncated=trunc1 | q.to(t.uint8), dones=(own | q).to(t.uint8), decoded=att._rows.clone(),
                 invalid_action=invalid, cyber_step_executed=info["cyber_step_executed"], network_availability=info["network_availability"].clone(),
                 step_count=info["step_count"].clone(), episode_return=info["episode_return"], episode_length=info["episode_length"],
                 episode_valid_actions=v0 + ~invalid, episode_invalid_actions=i0 + invalid)
        for k in att._obs:                                     # terminal rows: the live row as it stands (an intercepted action: the old one)
            att._terminal[k].copy_(t.where(self._rows(forced, att._obs[k]), att._obs[k], att._terminal[k]))
        eng.reset(forced)
        eng.observe(att._obs, env_mask=forced)                 # fresh rows and a fresh digest
        keep = ~forced
        att.timesteps.mul_(keep)
        att.valid_action_count.mul_(keep)
        att.invalid_action_count.mul_(keep)
        att.episode_returns.copy_(t.where(forced, t.zeros_like(att.episode_returns), att.episode_returns))      # (+0.0, not -x * 0)
        att.has_cyber_reward.logical_and_(keep)
        if with_mask:
            self.mask = att.action_masks_packed()              # of the observation the attacker now holds; stands through a defender-side reset
        n = (own | q) & ~q                                     # the attacker's reset notifies the defender only when it had not been asked
        # ---- defender half on the state as it stands ----
        _, r2, term2, trunc2, dinfo = dfd.step(a2)
        r2 = t.where(n, -(r1.double()), r2)
        trunc2 = trunc2 | n.to(t.uint8)
        done2 = (term2 | trunc2) != 0
        ret = self.defender_returns + r2
        d = dict(reward=r2, terminated=term2, truncated=trunc2, dones=done2.to(t.uint8), evicted=dfd._evicted.clone(), episode_return=ret,
                 episode_length=dfd.timesteps.clone(), episode_valid_actions=dfd.valid_action_count.clone(),
                 episode_invalid_actions=dfd.invalid_action_count.clone())
        d.update(dinfo)
        for k, v in dfd.observation.items():
            self.terminal[k].copy_(v)
        eng.reset(done2)                                       # the second cyber_env.reset(): discards what the defender just did
        dfd.reset(done2)                                       # counters, prev_availability, the fresh observation; the attacker's rows stand
        self.defender_returns = t.where(done2, t.zeros_like(ret), ret)
        self.request = done2 & ~n
        return a, d
