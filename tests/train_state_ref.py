"""The views of tests/test_train_state_gpu.py and the condition they must meet: consecutive steps
read mostly different point rows, and the last step reads rows that slept since the first."""
import numpy as np
import torch

from helpers import make_view

# (yaw, h, w): ray counts 192, 63, 192, 110 -- another batch size at every step, the first one again at the third
VIEWS = ((30.0, 12, 16), (150.0, 7, 9), (270.0, 12, 16), (30.0, 10, 11))
PITCH = -8.0
FIFTH_VIEW = (200.0, 9, 13)   # seen by no training step


def view(i):
    yaw, h, w = VIEWS[i] if i < len(VIEWS) else FIFTH_VIEW
    return make_view(h, w, yaw=yaw, pitch=PITCH)


def touched_from_pidx(pidx):
    """The distinct rows a step reads: its samples' neighbours and row 0 (the empty slots' conf)."""
    p = torch.as_tensor(np.asarray(pidx)).reshape(-1).long()
    return torch.unique(torch.cat([p[p >= 0], torch.zeros(1, dtype=torch.long)]))


def check_condition(touched):
    """touched[i]: sorted distinct rows of step i + 1.  Each of steps 2-4 reads at least 20 % rows the step
    before it did not touch; step 4 reads a row step 1 touched and steps 2-3 did not.  Returns the fresh
    fractions and the sleepers."""
    fresh = []
    for i in range(1, len(touched)):
        new = touched[i][~torch.isin(touched[i], touched[i - 1])]
        fresh.append(new.numel() / max(touched[i].numel(), 1))
        assert fresh[-1] >= 0.2, (i + 1, fresh)
    between = torch.cat([touched[1], touched[2]])
    sl = touched[3][torch.isin(touched[3], touched[0]) & ~torch.isin(touched[3], between)]
    assert sl.numel() >= 1
    return fresh, sl
