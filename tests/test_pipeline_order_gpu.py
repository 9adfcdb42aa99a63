"""What a ``submit`` of the three runners of madm_amd/pipeline.py enqueues, and in which order: event records, stream waits,
asynchronous input copies, graph replays, the range-probe copy.  The order is performance-relevant (one
extra wait, or streams created in another order, costs 10 - 30 % of the throughput) and invisible to the parity tests, so the
traces of ``2 * n_slots + 1`` submits + ``drain()`` per case are pinned to tests/golden/pipeline_submit_order.json
(tests/pipeline_trace.py wrote it and says how).  A change to the file is a change to what the device sees per submit: measure it."""
import json
import os

import pytest
import torch

import pipeline_trace

pytestmark = pytest.mark.gpu

EXTRACTOR_CASES = ["extractor_u3_device", "extractor_u3_host", "extractor_u3_slots6", "extractor_u2_nosync_norange"]
INFERENCE_CASES = ["graphed_s4_host_device", "staged_inference_u2_slots6"]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_submit_order.json")) as f:
        z = json.load(f)
    assert tuple(z["image_hw"]) == pipeline_trace.IMAGE_HW
    return z["cases"]


@pytest.fixture(scope="module")
def extractor_traces(cuda):
    return pipeline_trace.extractor_cases(pipeline_trace.build_extractor())


@pytest.fixture(scope="module")
def inference_traces(cuda):
    from test_eval_gpu import _build_product
    return pipeline_trace.inference_cases(_build_product("DEPTH", torch.float16))


def _assert_same(got, want, case):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{case}: call #{i} is {a}, the pinned order has {b} (before it: {got[max(0, i - 4):i]})"
    assert len(got) == len(want), f"{case}: {len(got)} calls, the pinned order has {len(want)}"


@pytest.mark.parametrize("case", EXTRACTOR_CASES)
def test_extractor_submit_order(extractor_traces, golden, case):
    _assert_same(extractor_traces[case], golden[case], case)


@pytest.mark.parametrize("case", INFERENCE_CASES)
def test_inference_submit_order(inference_traces, golden, case):
    _assert_same(inference_traces[case], golden[case], case)


def test_golden_covers_the_cases(golden):
    assert sorted(golden) == sorted(EXTRACTOR_CASES + INFERENCE_CASES)
    for case, log in golden.items():
        assert sum(e[0] == "replay" for e in log) > 0 and log[-1][0] in ("synchronize", "copy_", "record"), case
