"""tests/test_outer_parent.py on gfx950: every output of the outer layer stays bitwise equal to the recording made
with the product library of the commit before its unification (the "gpu/" arrays of tests/golden/outer_parent.npz)."""
import pytest

from test_outer_parent import check_bitwise_equal_to_parent

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def test_device_outputs_bitwise_equal_to_parent():
    check_bitwise_equal_to_parent("gpu")
