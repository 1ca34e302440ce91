"""
The batch driver, mode by mode, against the recorded behaviour of the five hand-written loops it replaced
(tests/golden/batch_driver_traces.json, written by tests/golden/gen_batch_driver_traces.py on the commit before the change):
every detector call with its names and keyword arguments, every on_results, every checkpoint, where each ring slot was
released, the printed lines and the results -- for load_and_run_detector_batch in-line, with loader threads and with the
shared-memory ring, and for process_video.run_detector_on_frames.  No GPU: a recording stub detector; the ring cases spawn one
loader process each.
"""

import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location('gen_batch_driver_traces', os.path.join(GOLDEN, 'gen_batch_driver_traces.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope='module')
def golden():
    with open(gen.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(list(gen.BATCH_CASES) + list(gen.VIDEO_CASES))


@pytest.mark.parametrize('case', list(gen.BATCH_CASES))
def test_load_and_run_detector_batch_trace(case, golden, tmp_path):
    trace, slot_errors = gen.record_batch_case(case, str(tmp_path))
    assert trace == golden[case]
    assert slot_errors == []                # every slot handed out was released exactly once
    if 'feed' in trace:
        handed_out = sum(trace['feed'].get(k, 0) for k in ('slot', 'jpeg', 'scan'))
        assert sum(1 for e in trace['events'] if e[0] == 'release') == handed_out
    if 'max_outstanding' in trace:
        assert trace['max_outstanding'] <= 2


@pytest.mark.parametrize('case', list(gen.VIDEO_CASES))
def test_run_detector_on_frames_trace(case, golden):
    trace = gen.record_video_case(case)
    assert trace == golden[case]
    if case.endswith('raises'):
        assert trace['raised'] == 'RuntimeError: simulated device failure'
        calls = [e[1] for e in trace['events'] if e[0] == 'call']
        assert calls.count('finish_batch') == 2 and calls[-1] == 'finish_batch'      # the second finish_batch raised, out of the function
    else:
        assert trace['raised'] is None
        assert [f for e in trace['events'] if e[0] == 'take' for f in e[1]] == trace['frame_filenames']
    if 'max_outstanding' in trace:
        assert trace['max_outstanding'] <= 2
