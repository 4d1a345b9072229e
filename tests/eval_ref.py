"""The episode tracker of ``marlnav_rollout_evaluate`` (include/marlnav.h)
restated in torch fp64, one call per step: the loop side of
tests/test_evaluate_gpu.py and, on a hand-written table, the subject of
tests/test_evaluate_cpu.py. Every operation is elementwise on its own env, in
step order, with one rounding per operation, as the kernel's."""
import math

import torch

PER_ENV = ("cur_return", "cur_len", "whole", "ep_count", "ret_sum", "ret_sqsum", "ret_min",
           "ret_max", "len_sum", "partial_count")


class EpisodeTracker(object):
    """``step_num`` (P,): the env's ``_step_num`` before the first step; an
    env that enters mid-episode (``step_num != 0``) closes a partial episode
    first."""

    def __init__(self, step_num):
        P, dev = step_num.shape[0], step_num.device
        z = lambda dtype: torch.zeros(P, dtype=dtype, device=dev)
        self.cur_return, self.cur_len = z(torch.float64), z(torch.int32)
        self.whole = step_num == 0
        self.ep_count, self.partial_count = z(torch.int32), z(torch.int32)
        self.ret_sum, self.ret_sqsum, self.len_sum = z(torch.float64), z(torch.float64), z(torch.int64)
        self.ret_min = torch.full((P,), math.inf, dtype=torch.float64, device=dev)
        self.ret_max = torch.full((P,), -math.inf, dtype=torch.float64, device=dev)

    def step(self, reward, terminated, truncated):
        """After a step: its reward (P,) fp32 and flags (P,) bool."""
        ret = self.cur_return + reward.double()
        length = self.cur_len + 1
        done = torch.logical_or(terminated, truncated)      # models.py:117
        closed = done & self.whole
        self.ep_count = self.ep_count + closed.int()
        self.ret_sum = torch.where(closed, self.ret_sum + ret, self.ret_sum)
        self.ret_sqsum = torch.where(closed, self.ret_sqsum + ret * ret, self.ret_sqsum)
        self.len_sum = torch.where(closed, self.len_sum + length, self.len_sum)
        self.ret_min = torch.where(closed & (ret < self.ret_min), ret, self.ret_min)
        self.ret_max = torch.where(closed & (ret > self.ret_max), ret, self.ret_max)
        self.partial_count = self.partial_count + (done & ~self.whole).int()
        self.cur_return = torch.where(done, torch.zeros_like(ret), ret)
        self.cur_len = torch.where(done, torch.zeros_like(length), length)
        self.whole = self.whole | done

    def totals(self):
        """(episodes, partials, len_sum) as ints and (ret_sum, ret_sqsum, min,
        max) as floats, summed by torch."""
        return ((int(self.ep_count.sum()), int(self.partial_count.sum()), int(self.len_sum.sum())),
                (float(self.ret_sum.sum()), float(self.ret_sqsum.sum()),
                 float(self.ret_min.min()), float(self.ret_max.max())))
