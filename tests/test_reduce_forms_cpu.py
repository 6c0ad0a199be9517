"""CPU suite: the order of the slab reductions as documented (csrc/gemm.hip: even slabs in one chain, odd slabs in the other, each in
increasing index, then scale) restated in float32 numpy -- and proof that the inputs of test_reduce_forms_gpu.py can tell that order
from a single sequential chain, so the bit-for-bit comparison on the GPU means something."""
import numpy as np
import pytest

import reduce_forms_common as C


def test_restatement_is_the_documented_order_on_a_hand_example():
    # 1e8 + 1 loses the 1 in float32: the two chains keep it where one chain drops it
    slabs = np.array([[1e8], [1.0], [-1e8], [1.0]], np.float32)
    assert C.two_chains(slabs, 1.0)[0] == np.float32(2.0)          # (1e8 - 1e8) + (1 + 1)
    assert C.one_chain(slabs, 1.0)[0] == np.float32(1.0)           # ((1e8 + 1) - 1e8) + 1
    assert C.two_chains(slabs[:1], 0.5)[0] == np.float32(5e7)
    assert C.two_chains(np.zeros((3, 2), np.float32), 1.0).tobytes() == np.zeros(2, np.float32).tobytes()     # +0.0, not -0.0


def test_inputs_have_mixed_magnitudes_and_both_signs():
    x = C.Case(16, 1024).slabs()
    assert x.dtype == np.float32 and np.isfinite(x).all()
    assert 1e-3 <= np.abs(x).min() < 1e-2 and 1e2 < np.abs(x).max() <= 1e3
    assert 0.4 < (x > 0).mean() < 0.6


@pytest.mark.parametrize("scale", [1.0, 1.0 / 32])
def test_every_vec_case_with_four_slabs_or_more_tells_the_two_orders_apart(scale):
    cases = [c for ns in C.SLABS for c in C.grid_cases(ns)] + C.odd_cases() + C.mixed24()
    vec = [c for c in cases if c.vec and c.ns >= 4]
    assert len(vec) >= 50
    for c in vec:
        x = c.slabs()[:, :c.count]
        a, b = C.two_chains(x, scale), C.one_chain(x, scale)
        assert (a.view(np.int32) != b.view(np.int32)).any(), c.name


def test_cases_cover_what_the_kernel_branches_on():
    cases = [c for ns in C.SLABS for c in C.grid_cases(ns)] + C.odd_cases() + C.mixed24()
    assert {c.ns for c in cases} >= set(C.SLABS) and {c.count for c in cases} >= set(C.COUNTS)
    assert any(c.src_off and not c.dst_off for c in cases) and any(c.dst_off and not c.src_off for c in cases)
    assert any(c.stride > c.count and c.vec for c in cases) and any(c.stride > c.count and not c.vec for c in cases)
    m = C.mixed24()
    assert len(m) == 24 and any(c.vec for c in m) and any(not c.vec for c in m) and len({c.name for c in m}) == 24
