"""CPU checks of the batched TrainingUpdate trace builder's boundary
(zkp_build_training_update_traces) and of the mask stream it makes on the device, as the
host entry zkp_pcg64_masks restates it: numpy's PCG64 draw, bit for bit."""
import ctypes

import numpy as np
import pytest

from test_abi import header_functions
from test_training import tu_prover
from zk_stark_project_amd import TrainingUpdateProver, _native

NEW = ["zkp_build_training_update_traces", "zkp_pcg64_masks"]
SEEDS = [0, 1, 2**63 - 1, 123456789]
ROWS = 96  # three tiles of 32 rows x 120 masks


def test_declared_and_exported():
    L = _native.load()
    for name in NEW:
        assert name in header_functions()
        assert name in _native.EXPORTED
        assert hasattr(L, name)


def test_python_entries_exist():
    assert callable(getattr(_native.Context, "build_training_update_traces", None))
    assert callable(getattr(TrainingUpdateProver, "build_traces_device", None))


def test_unequal_shapes_refused_before_any_context_is_used():
    a, b = tu_prover(1, seed=1), tu_prover(3, seed=2)
    with pytest.raises(ValueError):
        TrainingUpdateProver.build_traces_device([a, b], ctx=object())
    c = tu_prover(1, seed=3)
    c.trace_length = 256
    with pytest.raises(ValueError):
        TrainingUpdateProver.build_traces_device([a, c], ctx=object())
    assert TrainingUpdateProver.build_traces_device([], ctx=object()) == []


def test_client_struct_matches_header():
    """4 pointers, 2 felts, 1 pointer, 2 x 2 u64, 3 pointers: no padding on a 64-bit ABI."""
    assert ctypes.sizeof(_native.TrainingClientC) == 4 * 8 + 2 * 16 + 8 + 4 * 8 + 3 * 8


def test_null_context_rejected():
    L = _native.load()
    clients = (_native.TrainingClientC * 1)()
    assert L.zkp_build_training_update_traces(None, clients, 1, 0, 16) == 9  # ZKP_ERR_ARGUMENT
    assert L.zkp_build_training_update_traces(None, None, 0, 0, 16) == 9


def test_pcg_null_pointers_rejected():
    L = _native.load()
    two = (ctypes.c_uint64 * 2)(1, 2)
    out = (ctypes.c_uint64 * 4)()
    assert L.zkp_pcg64_masks(None, two, 0, 4, out) == 9
    assert L.zkp_pcg64_masks(two, None, 0, 4, out) == 9
    assert L.zkp_pcg64_masks(two, two, 0, 4, None) == 9
    assert L.zkp_pcg64_masks(two, two, 0, 4, out) == 0


@pytest.fixture(scope="module", params=SEEDS)
def draw(request):
    seed = request.param
    ref = np.random.default_rng(seed).integers(0, 1 << 64, size=(ROWS, 120), dtype=np.uint64, endpoint=False)
    return _native.pcg64_state(seed), ref.ravel()


def test_stream_from_index_zero(draw):
    (state, inc), ref = draw
    assert np.array_equal(_native.pcg64_masks(state, inc, 0, ref.size), ref)


# the last value of a tile and the first of the next (3839, 3840), around a row's end (119,
# 120, 239), mid-row, and the last value of the draw
@pytest.mark.parametrize("first,count", [(3839, 2), (3840, 3840), (119, 1), (120, 120), (239, 250), (1000, 1),
                                         (1919, 2), (ROWS * 120 - 1, 1), (5, 0)])
def test_stream_from_first_index(draw, first, count):
    (state, inc), ref = draw
    assert np.array_equal(_native.pcg64_masks(state, inc, first, count), ref[first:first + count])


def test_seed_state_is_a_fresh_pcg64():
    state, inc = _native.pcg64_state(7)
    st = np.random.default_rng(7).bit_generator.state
    assert (state, inc) == (st["state"]["state"], st["state"]["inc"]) and st["has_uint32"] == 0
    assert inc & 1  # an LCG increment is odd


def test_far_index_equals_stepping():
    """Jump-ahead past 2^32 against the same index reached from a nearer one by stepping."""
    state, inc = _native.pcg64_state(3)
    far = (1 << 33) + 12345
    a = _native.pcg64_masks(state, inc, far, 4)
    b = _native.pcg64_masks(state, inc, far - 1000, 1004)[1000:]
    assert np.array_equal(a, b)
