"""launch_opt_moments (csrc/optim_moments.hip) refuses exactly as the build before its row forms became one table (ROW_FORMS,
resolve_row_form): every never-launching descriptor of opt_moments_refusal_cases gets the return code and the nasrec_last_error text
recorded from that build (tests/golden/opt_moments_refusals_parent.json, written by tools/record_opt_moments_refusals.py) — so every
refusal kept its text, its code and, where two apply, its precedence.  Host only: nothing is launched.  The pointer refusals that
need B > 0 are held by the REFUSALS tests of the *_kernel_gpu.py files."""
import json
import os

import opt_moments_refusal_cases as R
from nasrec_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "opt_moments_refusals_parent.json")


def test_every_descriptor_is_refused_as_the_parent_refused_it():
    with open(GOLDEN) as f:
        gold = json.load(f)
    lib = L.load()
    cases = R.cases()
    answers = {block + " " + rest: a for block, rows in gold["answers"].items() for rest, a in rows.items()}
    assert len(cases) == 2800 + 350 * len(R.VARIANTS) and {k for k, _ in cases} == set(answers)
    wrong = []
    for key, d in cases:
        rc, msg = R.answer(lib, d)
        want_rc, want_msg = answers[key][0], gold["messages"][answers[key][1]]
        assert want_rc in (-1, -2)  # (the fixture holds refusals only)
        if (rc, msg) != (want_rc, want_msg):
            wrong.append((key, (rc, msg), (want_rc, want_msg)))
    assert not wrong, "%d of %d descriptors answered otherwise; the first: %r" % (len(wrong), len(cases), wrong[:5])
