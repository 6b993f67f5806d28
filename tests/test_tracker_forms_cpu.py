"""Every form of the multi-delta tracker on one 13-frame stub sequence, on the
CPU: without and with the feature cache, dense, and a second run after
reset(), bit for bit against an oracle that keeps its history in a Python
list (tests/tracker_forms_cases.py).  The sequence runs past t = 2L, into the
periodic part of the ring's index table, and exercises the point tracker's
history rings without the cache."""
import pytest
import torch

import tracker_forms_cases as C


@pytest.mark.parametrize("deltas", C.DELTAS)
def test_every_form_is_the_list_oracle(deltas):
    C.check_forms(deltas, torch.device("cpu"))
