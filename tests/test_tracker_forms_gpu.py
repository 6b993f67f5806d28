"""tests/test_tracker_forms_cpu.py on the GPU: the graphed trackers in every
form against the CPU oracle, bit for bit (the stub's flows and the rule's
arithmetic on them are exact on both devices, as in tests/test_multi_flow_gpu.py)."""
import pytest

import tracker_forms_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("deltas", C.DELTAS)
def test_every_form_is_the_list_oracle(cuda, deltas):
    C.check_forms(deltas, cuda)
