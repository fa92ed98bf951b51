"""Record how launch_opt_moments answers the never-launching descriptors of tests/opt_moments_refusal_cases.py:

    NASREC_HIP_LIB=<the library of the commit to record> python tools/record_opt_moments_refusals.py OUT.json

Host only (no device is touched: every descriptor is refused before a launch, which this recorder asserts).  The committed
tests/golden/opt_moments_refusals_parent.json is this file's output for the build of the commit before the row forms became one
table (ROW_FORMS, csrc/optim_moments.hip); tests/test_opt_moments_refusals_cpu.py holds the current build to it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import opt_moments_refusal_cases as R  # noqa: E402
from nasrec_amd import _lib as L  # noqa: E402


def main(out):
    lib = L.load()
    messages, answers = [], {}
    for key, d in R.cases():
        rc, msg = R.answer(lib, d)
        assert rc in (-1, -2) and msg, "descriptor %r was not refused (rc %d): it may have launched" % (key, rc)
        if msg not in messages:
            messages.append(msg)
        block, _, rest = key.partition(" p")  # (one line of the file per (algo, sparse_rows, table_algo))
        answers.setdefault(block, {})["p" + rest] = [rc, messages.index(msg)]
    dump = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    with open(out, "w") as f:
        f.write('{"messages": [\n%s\n],\n"answers": {\n%s\n}}\n' % (",\n".join(dump(m) for m in messages),
                                                                   ",\n".join("%s: %s" % (dump(b), dump(a)) for b, a in answers.items())))
    print("%d descriptors, all refused; %d distinct messages" % (sum(map(len, answers.values())), len(messages)))


if __name__ == "__main__":
    main(sys.argv[1])
