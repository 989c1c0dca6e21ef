"""examples/logistic_mcmc_eval.py --curve 4 and examples/group_shapley.py at small settings with --summary: they print a finite
worst R-hat and smallest ESS per coreset size / for the run, and every other figure they print -- accuracies, log-likelihoods,
steps, Shapley values; not the wall times -- is that of a run without the flag.  The examples are what these tests are about, so
they are started as programs."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', script)] + args, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr[-3000:]
    return res.stdout.splitlines()


def _untimed(lines):
    """the lines with their wall times blanked ('1.23 s', '4.5 ms'), the summary's own lines left out"""
    return [re.sub(r'\d+\.\d+ m?s\b', 'T', ln) for ln in lines if 'R-hat' not in ln]


def _figures(line):
    return [float(v) for v in re.findall(r'R-hat (\S+?)[, ]', line) + re.findall(r'smallest ESS (\S+) of', line)]


def test_logistic_mcmc_eval_prints_rhat_and_ess_beside_unchanged_scores():
    args = ['--n', '3000', '--n-test', '300', '--d', '4', '--m', '12', '--samples', '32', '--warmup', '10', '--chains', '4', '--proj-dim', '40',
            '--curve', '4']
    plain, with_ = _run('logistic_mcmc_eval.py', args), _run('logistic_mcmc_eval.py', args + ['--summary'])
    chains = [ln for ln in with_ if 'R-hat' in ln]
    assert len(chains) == 4 and not any('R-hat' in ln for ln in plain)
    for ln in chains:
        rhat, ess = _figures(ln)
        assert 0.5 < rhat < 100. and math.isfinite(ess), ln      # (finite: 32 draws a chain say little more about an ESS)
    assert _untimed(with_) == _untimed(plain)


def test_group_shapley_prints_the_runs_worst_rhat():
    args = ['--groups', '6', '--d', '3', '--n-test', '200', '--perms', '3', '--max-groups', '3', '--select', '2', '--rand-trials', '2']
    plain, with_ = _run('group_shapley.py', args), _run('group_shapley.py', args + ['--summary'])
    chains = [ln for ln in with_ if 'R-hat' in ln]
    assert len(chains) == 1 and not any('R-hat' in ln for ln in plain)
    rhat, ess = _figures(chains[0])
    assert 0.5 < rhat < 100. and math.isfinite(ess), chains[0]
    assert _untimed(with_) == _untimed(plain)
