"""The protocol of the chunked device runs (csrc/bc_run.h) and the packed batch (csrc/bc_batch.h) on the CPU:
tests/run_protocol_harness.cpp built as a program of its own with AddressSanitizer and UBSan and run directly.  Every
transition of the run state with its exact message for both nouns, the row_ptr walk and the splitter of unmarked runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, MARKED, BAD = 0, 1, 2          # BC_OK, BC_NUMERICAL_PRECISION, BC_INVALID_ARGUMENT
KINDS = [('bc_vi_optimize', 'steps'), ('bc_hmc_small', 'iterations')]


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('run_protocol') / 'run_protocol_harness')
    cmd = ['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           os.path.join(ROOT, 'tests', 'run_protocol_harness.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == '', (args, out.returncode, out.stderr[-2000:])
    return out.stdout.rstrip('\n').split('|')


def state(active=1, pending=0, failed=0, done=0, total=5):
    return [active, pending, failed, done, total]


# ---------------------------------------------------------------- the run state
def test_open_resets_whatever_the_last_run_left(harness):
    assert run(harness, 'open', *state(0, 1, 1, 4, 5), 9) == ['1 0 0 0 9']


@pytest.mark.parametrize('name,noun', KINDS)
def test_admit(harness, name, noun):
    who = name + '_chunk_begin'
    none_open = [str(BAD), who + ': bad argument, or no run is open']

    def admit(st, args_ok=1, k=1):
        return run(harness, 'admit', name, noun, *st, args_ok, k)
    assert admit(['null']) == none_open                                  # before any _begin
    assert admit(state(active=0)) == none_open                           # after _end
    assert admit(state(), args_ok=0) == none_open
    assert admit(state(), k=0) == none_open and admit(state(), k=-3) == none_open
    assert admit(state(pending=1)) == [str(BAD), '%s: a chunk is pending (call %s_chunk_end first)' % (who, name)]
    assert admit(state(failed=1)) == [str(BAD), '%s: the run has failed (call %s_end)' % (who, name)]
    # today's order: a pending chunk is named before a failed run, a failed run before the length
    assert admit(state(pending=1, failed=1, done=5))[1].endswith('_chunk_end first)')
    assert admit(state(failed=1, done=5))[1].endswith('_end)')
    assert admit(state(done=2), k=3) == [str(OK), '']                    # done + k = total
    assert admit(state(done=2), k=4) == [str(BAD), "%s: 4 %s after 2 exceed the run's 5" % (who, noun)]
    assert admit(state(done=0, total=3000000000), k=2147483647) == [str(OK), '']
    assert admit(state(done=2999999999, total=3000000000), k=2) == [str(BAD), "%s: 2 %s after 2999999999 exceed the run's 3000000000" % (who, noun)]


@pytest.mark.parametrize('who', ['bc_hmc_small_chunk_end', 'bc_score_chunk_end'])
def test_a_chunk_is_pending_to_be_ended(harness, who):
    refused = [str(BAD), who + ': no chunk is pending']
    assert run(harness, 'pending', who, 'null') == refused
    assert run(harness, 'pending', who, *state(active=0, pending=1)) == refused
    assert run(harness, 'pending', who, *state(pending=0)) == refused
    assert run(harness, 'pending', who, *state(pending=1)) == [str(OK), '']
    assert run(harness, 'pending', who, *state(pending=1, failed=1)) == [str(OK), '']      # (a failed run's chunk is still waited for)


@pytest.mark.parametrize('name,noun', KINDS)
def test_close(harness, name, noun):
    refused = [str(BAD), name + '_end: no run is open', '0', '0 0']
    assert run(harness, 'close', name, noun, 'null') == refused
    assert run(harness, 'close', name, noun, *state(active=0)) == refused
    assert run(harness, 'close', name, noun, *state(pending=0, done=3)) == [str(OK), '', '0', '0 0']
    assert run(harness, 'close', name, noun, *state(pending=1, done=3)) == [str(OK), '', '1', '0 0']      # abandoned mid-chunk


@pytest.mark.parametrize('name,noun', KINDS)
def test_results_are_fetched_from_a_complete_run_only(harness, name, noun):
    def complete(st, was_pending=0):
        return run(harness, 'complete', name, noun, *st, was_pending, 'no weights')
    msg = name + '_end: the run is not complete (%d of 5 ' + noun + '%s): no weights'
    assert complete(state(active=0, done=5)) == [str(OK), '']
    assert complete(state(active=0, done=4)) == [str(BAD), msg % (4, '')]
    assert complete(state(active=0, done=0)) == [str(BAD), msg % (0, '')]
    assert complete(state(active=0, failed=1, done=5)) == [str(BAD), msg % (5, ', failed')]
    assert complete(state(active=0, done=5), was_pending=1) == [str(BAD), msg % (5, '')]
    assert complete(state(active=0, failed=1, done=3), was_pending=1) == [str(BAD), msg % (3, ', failed')]


# ---------------------------------------------------------------- the packed batch
def walk(harness, row_ptr, cap=1 << 24, holds='rows', who='bc_laplace_small'):
    rc, largest, msg = run(harness, 'walk', who, cap, holds, *row_ptr)
    return int(rc), int(largest), msg


def test_the_row_ptr_walk(harness):
    assert walk(harness, [0, 1, 3]) == (OK, 2, '')
    assert walk(harness, [1, 2, 3]) == (BAD, -1, 'bc_laplace_small: row_ptr[0] must be 0, got 1')
    for row_ptr, p, n in (([0, 2, 2], 1, 0), ([0, 8, 1, 72], 1, -7)):
        rc, _, msg = walk(harness, row_ptr, who='bc_hmc_small_begin')
        assert rc == BAD and msg == 'bc_hmc_small_begin: problem %d has %d rows, 1 .. 16777216 are served (row_ptr must increase strictly: ' \
            'row_ptr[%d] = %d, row_ptr[%d] = %d)' % (p, n, p, row_ptr[p], p + 1, row_ptr[p + 1])
    assert walk(harness, [0, 4096], cap=4096, holds='points', who='bc_psvi_many_begin') == (OK, 4096, '')
    rc, _, msg = walk(harness, [0, 3, 4100], cap=4096, holds='points', who='bc_psvi_many_begin')
    assert rc == BAD and msg.startswith('bc_psvi_many_begin: problem 1 has 4097 points, 1 .. 4096 are served (row_ptr')
    assert walk(harness, [0, 5, 6, 16]) == (OK, 10, '')


@pytest.mark.parametrize('flags,runs', [((0, 0, 0, 0), [(0, 4)]), ((1, 1, 1), []), ((1, 0, 0), [(1, 3)]), ((0, 0, 3), [(0, 2)]),
                                        ((0, 1, 0, 1, 0), [(0, 1), (2, 3), (4, 5)]), ((1, 0, 1, 0), [(1, 2), (3, 4)]), ((0,), [(0, 1)]),
                                        ((1, 1, 0, 1), [(2, 3)]), ((-1, 0, 0, 2, 2, 0, 0, 0), [(1, 3), (5, 8)])])
def test_unmarked_problems_are_handed_out_in_maximal_runs(harness, flags, runs):
    status, got = run(harness, 'split', *flags)
    got = [tuple(int(v) for v in r.split(':')) for r in got.split()]
    assert [int(v) for v in status.split()] == [MARKED if f else OK for f in flags]
    assert got == runs
    # every unmarked index exactly once, no marked one, and no two runs touch (they are maximal)
    covered = [p for a, b in got for p in range(a, b)]
    assert covered == [p for p, f in enumerate(flags) if not f]
    assert all(b0 < a1 for (_, b0), (a1, _) in zip(got, got[1:]))
