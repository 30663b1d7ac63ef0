"""Argument validation of fused_expert_nll_occupancy: the range rules run
before the runtime is asked anything, so they need no GPU and must raise a
RuntimeError that names the argument."""

import pytest

from spark_gp_amd import _hip_ext as ext

RULES = [
    ("k = 0", lambda: ext.fused_expert_nll_occupancy(0, 4), "k"),
    ("k = 129", lambda: ext.fused_expert_nll_occupancy(129, 4), "k"),
    ("d = 0", lambda: ext.fused_expert_nll_occupancy(8, 0), "d"),
    ("d = 129", lambda: ext.fused_expert_nll_occupancy(8, 129), "d"),
]


@pytest.mark.parametrize("call,name", [r[1:] for r in RULES],
                         ids=[r[0] for r in RULES])
def test_rule_names_its_argument(call, name):
    with pytest.raises(RuntimeError, match=rf"^{name}\b"):
        call()


def test_non_integer_arguments_are_a_type_error():
    with pytest.raises(TypeError):
        ext.fused_expert_nll_occupancy(100.5, 32)
    with pytest.raises(TypeError):
        ext.fused_expert_nll_occupancy(100)
