"""The two-agent TRAINING turn's hand-shake in numpy: rules 1-3 of mcbs_two_agent_train_step (include/mcbs.h) — the request byte, `n`,
the override, what is cleared when — as marl_algorithm.collect_rollouts' two DummyVecEnv resets produce them on the reference's wrappers
(attack_wrapper.py:341-346, 433-451; defend_wrapper.py:267-273, 446-463).  The environment step, the defender's turn and its reward
shaping are NOT restated here: `attacker()` and `defender()` are fed their per-step results (recorded from the reference in
tests/golden/wrap_training_*.npz, or computed by the existing calls on the device) and return what the turn makes of them.  Shared by
tests/test_training_host.py (against the fixtures) and tests/test_gpu_two_agent_training.py (inside the composition from existing calls)."""
import numpy as np


class TrainingBook:
    def __init__(self, n_envs: int, attacker_max_timesteps: int, defender_max_timesteps: int):
        E = self.n_envs = int(n_envs)
        self.a_max, self.d_max = int(attacker_max_timesteps), int(defender_max_timesteps)
        self.request = np.zeros(E, bool)                   # attacker_reset_request
        self.a_timesteps = np.zeros(E, np.int32)
        self.a_valid = np.zeros(E, np.int64)
        self.a_invalid = np.zeros(E, np.int64)
        self.a_return = np.zeros(E, np.float64)
        self.d_timesteps = np.zeros(E, np.int32)
        self.d_valid = np.zeros(E, np.int64)
        self.d_invalid = np.zeros(E, np.int64)
        self.d_return = np.zeros(E, np.float64)
        self.reinitialised = np.zeros(E, np.int64)         # re-initialisations so far: S.episode's increments
        self.a_last_valid = np.zeros(E, np.int64)          # the wrappers' last_*_action_count: the counts of the episode that ended last
        self.a_last_invalid = np.zeros(E, np.int64)
        self.d_last_valid = np.zeros(E, np.int64)
        self.d_last_invalid = np.zeros(E, np.int64)
        self._n = np.zeros(E, bool)
        self._r1 = np.zeros(E, np.float32)

    def attacker(self, reward, terminated, invalid):
        """reward: float32 [E], the step's reward with the modifier of an intercepted action; terminated, invalid: flags [E].
        -> dict: truncated, dones, notify (n), requested (q), episode_return / length / valid / invalid including this step"""
        reward = np.asarray(reward, np.float32)
        terminated, invalid = np.asarray(terminated) != 0, np.asarray(invalid) != 0
        q = self.request.copy()
        t = self.a_timesteps + 1
        truncated = (t >= self.a_max) | q                                       # attack_wrapper.py:341-346
        done = terminated | truncated
        valid, n_invalid = self.a_valid + ~invalid, self.a_invalid + invalid
        ret = self.a_return + reward.astype(np.float64)
        out = dict(truncated=truncated, dones=done, notify=done & ~q, requested=q, episode_return=ret, episode_length=t.astype(np.int32),
                   episode_valid_actions=valid, episode_invalid_actions=n_invalid)
        # DummyVecEnv resets the wrapper at once: counters cleared, the request consumed, the defender notified unless the attacker was asked
        self.a_timesteps = np.where(done, 0, t).astype(np.int32)
        self.a_valid, self.a_invalid = np.where(done, 0, valid), np.where(done, 0, n_invalid)
        self.a_return = np.where(done, 0.0, ret)
        self.a_last_valid, self.a_last_invalid = np.where(done, valid, self.a_last_valid), np.where(done, n_invalid, self.a_last_invalid)
        self.reinitialised += done
        self.request[:] = False
        self._n, self._r1 = done & ~q, reward
        return out

    def defender(self, reward, terminated, valid):
        """reward: float64 [E] and terminated [E] as the wrapper's shaping gives them for this step (on the state the attacker half left);
        valid [E]: the action's validity.  -> dict: reward, terminated, truncated, dones, request_step (n), episode outputs"""
        reward = np.asarray(reward, np.float64).copy()
        terminated, valid = np.asarray(terminated) != 0, np.asarray(valid) != 0
        n = self._n
        t = self.d_timesteps + 1
        truncated = (t >= self.d_max) | n                                       # defend_wrapper.py:269-273
        reward[n] = -self._r1[n].astype(np.float64)                             # overrides the shaped value, -0.0 included
        done = terminated | truncated
        n_valid, n_invalid = self.d_valid + valid, self.d_invalid + ~valid
        ret = self.d_return + reward
        out = dict(reward=reward, terminated=terminated, truncated=truncated, dones=done, request_step=n.copy(), episode_return=ret,
                   episode_length=t.astype(np.int32), episode_valid_actions=n_valid, episode_invalid_actions=n_invalid)
        self.d_timesteps = np.where(done, 0, t).astype(np.int32)
        self.d_valid, self.d_invalid = np.where(done, 0, n_valid), np.where(done, 0, n_invalid)
        self.d_return = np.where(done, 0.0, ret)
        self.d_last_valid, self.d_last_invalid = np.where(done, n_valid, self.d_last_valid), np.where(done, n_invalid, self.d_last_invalid)
        self.reinitialised += done                                              # the reference's second cyber_env.reset()
        self.request = done & ~n                                                # defend_wrapper.py:446-447: the attacker is asked next turn
        self._n = np.zeros(self.n_envs, bool)
        return out
