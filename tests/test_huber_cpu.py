"""keras-rl's finite delta_clip (the Huber TD loss), the parts that need no GPU: the float64 reference the GPU tests use, checked against
torch's own Huber loss; the agent surface accepting and validating delta_clip; its encoding in dq_td_job; the new C entry points."""
import ctypes
import importlib

import numpy as np
import pytest
import torch


def huber_c(x, delta):
    """keras-rl 0.4.2 huber_loss's gradient, float64: x clamped to [-delta, delta] by a compare (NaN stays NaN, +-inf gives +-delta)."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > delta, np.copysign(delta, x), x)


def huber_h(x, delta):
    """keras-rl 0.4.2 huber_loss, float64: 0.5 x^2 inside |x| <= delta, delta (|x| - 0.5 delta) beyond; delta = inf is exactly 0.5 x^2."""
    x = np.asarray(x, np.float64)
    if np.isinf(delta):
        return 0.5 * x * x
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > delta, delta * (np.abs(x) - 0.5 * delta), 0.5 * x * x)


def _points(delta):
    return np.array([0.0, -0.0, 0.3 * delta, -0.7 * delta, delta, -delta, np.nextafter(delta, 0), np.nextafter(delta, np.inf),
                     -np.nextafter(delta, np.inf), 1.5 * delta, -4.0 * delta, 1e6, -1e6, np.inf, -np.inf])


@pytest.mark.parametrize("delta", [0.05, 1.0, 7.5])
def test_reference_huber_equals_torch_huber_loss_and_its_gradient(delta):
    x = _points(delta)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ht = torch.nn.functional.huber_loss(xt, torch.zeros_like(xt), reduction="none", delta=delta)
    ht.sum().backward()
    finite = np.isfinite(x)
    np.testing.assert_array_equal(huber_h(x, delta)[finite], ht.detach().numpy()[finite])
    np.testing.assert_array_equal(huber_h(x, delta)[~finite], np.inf)
    np.testing.assert_array_equal(huber_c(x, delta), xt.grad.numpy())          # torch clamps +-inf to +-delta as well
    assert np.all(np.abs(huber_c(x, delta)) <= delta)
    # NaN propagates through both (the fmin / fmax form of the clamp would turn it into +-delta)
    assert np.isnan(huber_c(np.nan, delta)) and np.isnan(huber_h(np.nan, delta))
    assert np.isnan(huber_c(np.array([np.nan]), delta)).all()


def test_reference_huber_at_infinite_delta_is_the_squared_error():
    x = np.array([0.0, 1e-3, -2.5, 1e6, np.inf, -np.inf])
    np.testing.assert_array_equal(huber_h(x, np.inf), 0.5 * x * x)              # (no inf - inf anywhere: inf, not NaN, at x = +-inf)
    np.testing.assert_array_equal(huber_c(x, np.inf), x)


def _agent_parts(dq, rl_dqn=None):
    from importlib import import_module
    A = import_module("deepq-decoding_amd.agent")
    model = A.build_convolutional_nn([[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]], (4, 7, 7), 10)
    return A, model


def test_agent_accepts_finite_delta_clip(dq):
    A, model = _agent_parts(dq)
    agent = A.DQNAgent(model=model, nb_actions=10, memory=A.SequentialMemory(limit=1000, window_length=1), enable_dueling_network=True,
                       delta_clip=1.0)
    assert agent.delta_clip == 1.0 and agent.get_config()["delta_clip"] == 1.0
    assert np.isinf(A.DQNAgent(model=model, nb_actions=10, memory=A.SequentialMemory(limit=1000, window_length=1)).delta_clip)
    for bad in (0.0, -1.0, float("nan"), 1e-50):
        with pytest.raises(ValueError):
            A.DQNAgent(model=model, nb_actions=10, memory=A.SequentialMemory(limit=1000, window_length=1), delta_clip=bad)


def test_agent_accepts_finite_delta_clip_through_the_dropin_tree(dq):
    """A keras-rl driver script's own imports (rl.agents.dqn, rl.memory, keras.models) with DQNAgent(..., delta_clip=1.0)."""
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "deepq-decoding_amd", "dropin"))
    try:
        rl_dqn = importlib.import_module("rl.agents.dqn")
        rl_memory = importlib.import_module("rl.memory")
    finally:
        sys.path.pop(0)
    A = importlib.import_module("deepq-decoding_amd.agent")
    assert rl_dqn.DQNAgent is A.DQNAgent
    model = A.build_convolutional_nn([[64, 3, 2], [32, 2, 1], [32, 2, 1]], [[512, 0.2]], (4, 7, 7), 10)
    agent = rl_dqn.DQNAgent(model=model, nb_actions=10, memory=rl_memory.SequentialMemory(limit=1000, window_length=1), delta_clip=1.0,
                            enable_dueling_network=True, dueling_type="avg")
    assert agent.delta_clip == 1.0
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            rl_dqn.DQNAgent(model=model, nb_actions=10, memory=rl_memory.SequentialMemory(limit=1000, window_length=1), delta_clip=bad)


def test_td_job_encodes_delta_clip(dq):
    """dq_td_job.delta_clip: inf (and an absent key) -> 0, the zero-initialised struct every caller built before the field existed; finite -> itself."""
    Q = importlib.import_module("deepq-decoding_amd.qnet")
    base = dict(q_online_s1=None, q_target_s1=None, q_s0=torch.zeros(4, 3), reward=None, terminal=None, action=None, gamma=0.99)
    assert Q._td_job(base).delta_clip == 0.0
    assert Q._td_job(dict(base, delta_clip=np.inf)).delta_clip == 0.0
    assert Q._td_job(dict(base, delta_clip=None)).delta_clip == 0.0
    assert Q._td_job(dict(base, delta_clip=1.0)).delta_clip == 1.0
    assert Q._td_job(dict(base, delta_clip=0.05)).delta_clip == 0.05
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            Q._td_job(dict(base, delta_clip=bad))


def test_core_validates_delta_clip(dq):
    Q = importlib.import_module("deepq-decoding_amd.qnet")
    assert Q.check_delta_clip(np.inf) == np.inf and Q.check_delta_clip(1) == 1.0
    for bad in (0.0, -1.0, float("nan"), -np.inf):
        with pytest.raises(ValueError):
            Q.check_delta_clip(bad)


def test_new_entry_points_are_declared_exported_and_bound(dq):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "deepq_hip.h")).read()
    L = importlib.import_module("deepq-decoding_amd._lib")
    for name in ("dq_td_loss_grad_clip", "dq_td_step"):
        assert f"dq_status {name}(" in header
        assert name in L.SIGNATURES
        assert getattr(L.lib(), name) is not None
    assert L.lib().dq_version() >= 2
    assert L.TdJob._fields_[-1] == ("delta_clip", ctypes.c_double)
    assert L.lib().dq_struct_size(5) == ctypes.sizeof(L.TdJob)


def test_new_entry_points_refuse_invalid_delta_without_a_gpu(dq):
    """Argument checks happen on the host, before any launch: delta <= 0 or NaN is DQ_ERR_INVALID (dq_td_loss_grad_clip), and a job with a
    negative delta is refused by dq_td_step."""
    L = importlib.import_module("deepq-decoding_amd._lib")
    lib = L.lib()
    for bad in (0.0, -1.0, float("nan")):
        assert lib.dq_td_loss_grad_clip(None, None, None, None, 4, 3, 0.25, bad, None, None, None) == -1
        j = L.TdJob()
        j.delta_clip = bad if bad != 0.0 else -0.5
        assert lib.dq_td_step(ctypes.byref(j), None) == -1
        assert b"delta_clip" in lib.dq_last_error()
