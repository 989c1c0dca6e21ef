"""K1 on the device, element by element, against the long-double reference and the derived bound of tests/k1_cases.py: every
model id on every instance of the staged kernel and in the un-centred passes of S > 256 (STAGED), and on the Theta-resident
kernel (RESIDENT).  Phi, the row norms and the column sums must be finite and inside the bound; no element is left out.  The
worst |error| / bound of each case is printed (pytest -s) and recorded, per family, in tests/k1_cases.py."""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import k1_cases as K                                                             # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def bc():
    import beta_cores_amd as bc
    bc.default_context()
    return bc


def need_longdouble():
    if not K.LONGDOUBLE_OK:
        pytest.skip(K.LONGDOUBLE_WHY)


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count      # what project_r_grid sizes its grid by (ctx->n_cu)


def fixed(th):
    return lambda n, w, p: th


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize('case', K.STAGED, ids=['%s-n%d-d%d-S%d-%s' % c for c in K.STAGED])
def test_staged_case(bc, case):
    """The three model ids of the case's family through prj._run on resident rows: Phi, norms and column sums, every element."""
    need_longdouble()
    fam, n, d, S, kind = case
    inp, refs = K.case(*case)
    model, ids = K.model_and_ids(bc.likelihoods, fam, inp)
    prj = bc.DeviceBetaProjector(fixed(inp['th']), S, model)
    dd = bc.DeviceData(inp['Z'])
    os.environ.pop('BC_K1_STAGED', None)
    worst = []
    for mid, params in ids:
        phi = prj._run(dd, mid, params)
        got = (phi.to_host(), phi.norms(), phi.colsum())
        del phi
        assert got[0].shape == (n, S) and got[1].shape == (n,) and got[2].shape == (S,)
        assert all(np.isfinite(g).all() for g in got), (case, K.NAMES[mid])
        r = K.ratios(refs[mid], *got)
        worst.append((K.NAMES[mid], r))
    print('K1 bound %s instance %s: ' % ('-'.join(str(x) for x in case), K.instance(S)[0])
          + '; '.join('%s Phi %.3f norms %.3f colsum %.3f' % ((nm,) + r) for nm, r in worst))
    for nm, r in worst:
        assert max(r) <= 1., (case, nm, 'error / bound of (Phi, norms, column sums)', r)


@pytest.mark.parametrize('d,S', K.RESIDENT)
@pytest.mark.parametrize('fam', K.FAMILIES)
def test_resident_case(bc, fam, d, S):
    """k_project_r: n = 128 * 8 * n_cu + 77 rows ('wide' inputs), every model id that has a resident instance at this S (the
    logistic beta-likelihood is sent there with BC_K1_STAGED=-1); values and norms of 300-odd picked rows -- the group and tile
    edges, the ragged last group, the zero-feature rows -- inside the bound."""
    need_longdouble()
    n = K.resident_rows(n_cu())
    inp = K.resident_inputs(fam, n, d, S)
    assert inp['Z'].nbytes < 100e6
    pick = K.resident_pick(n, np.random.RandomState(d + S))
    model, ids = K.model_and_ids(bc.likelihoods, fam, inp)
    prj = bc.DeviceBetaProjector(fixed(inp['th']), S, model)
    dd = bc.DeviceData(inp['Z'])
    worst = []
    for mid, params in ids:
        if K.instance(S)[0] == '7' and mid in K.RESIDENT_NO_NT7:
            continue                               # no such instance: the staged kernel serves it, and test_staged_case holds that
        ref = K.reference(fam, mid, inp, rows=pick)
        K.check_conditions(fam, ref, 'wide')
        with env(BC_K1_STAGED=-1 if mid == 3 else 0):
            phi = prj._run(dd, mid, params)
            rows, norms = phi.rows(pick), phi.norms()
            del phi
        assert norms.shape == (n,) and np.isfinite(norms).all() and np.isfinite(rows).all()
        r = K.ratios(ref, rows, norms[pick])
        worst.append((K.NAMES[mid], r[:2]))
    print('K1 bound resident %s d=%d S=%d n=%d: ' % (fam, d, S, n) + '; '.join('%s Phi %.3f norms %.3f' % ((nm,) + r) for nm, r in worst))
    assert worst
    for nm, r in worst:
        assert max(r) <= 1., (fam, d, S, nm, 'error / bound of (Phi, norms)', r)
