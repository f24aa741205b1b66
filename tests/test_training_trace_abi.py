"""CPU checks of the TrainingUpdate device trace builder's boundary
(zkp_build_training_update_trace): declared, exported, rejects a null context like
its GlobalUpdate neighbour, and leaves the host path of get_pub_inputs as it was."""
import ctypes
import os

from test_abi import header_functions
from test_training import tu_prover
from zk_stark_project_amd import TrainingUpdateProver, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_and_exported():
    assert "zkp_build_training_update_trace" in header_functions()
    assert "zkp_build_training_update_trace" in _native.EXPORTED
    assert hasattr(_native.load(), "zkp_build_training_update_trace")


def test_null_context_rejected_like_global_update():
    L = _native.load()
    zero = _native.Felt(0, 0)
    gu = L.zkp_build_global_update_trace(None, None, None, None, 0, zero, 16, None, None)
    tu = L.zkp_build_training_update_trace(None, None, None, None, None, 0, zero, zero, None, 16, None, None, None)
    assert tu == gu == 9  # ZKP_ERR_ARGUMENT


def test_prover_has_device_builder():
    assert callable(getattr(TrainingUpdateProver, "build_trace_device", None))
    assert callable(getattr(_native.Context, "build_training_update_trace", None))


def test_pub_inputs_from_host_trace_unchanged():
    p = tu_prover(1, seed=3)
    tr = p.build_trace()
    pub = p.get_pub_inputs(tr)
    assert pub.initial_masked == [tr.get(c, 0) for c in range(120)]
    assert pub.final_masked == [tr.get(c, tr.length() - 1) for c in range(120)]
    e = pub.to_elements()
    assert len(e) == 240 + 4 + 9 + 6 and e[:120] == pub.initial_masked and e[120:240] == pub.final_masked
    assert pub.steps == tr.length() - 1 and pub.batch_size == 1
