#!/usr/bin/env python
"""Record the reference engine's results for tests/test_oracle_vs_ref.py as SHA-256 digests of their bits
(tests/golden/reference_digests.json), so that the restatement is checked bit for bit where oracle/_ref is not built.

Needs oracle/_ref (built by __graft_entry__.build() where the reference checkout exists):  python tests/golden/make_ref_digests.py
Every recorded result is also compared with the restatement's on the way; a mismatch records nothing."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import oracle  # noqa: E402
import test_oracle_vs_ref as T  # noqa: E402


def main():
    assert oracle.have_ref() and oracle.have_port(), "needs oracle/_ref and oracle/libelemoracle.so (run build() first)"
    out = {}
    for key in T.SCENARIOS:
        want = T.digest(T.run_scenario(key, T.ref))
        got, live = T.run_scenario(key, T.port, T.ref)
        assert T.digest(got) == want == T.digest(live), f"{key}: the restatement differs from the reference"
        out[key] = want
    with open(T.DIGESTS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} digests -> {os.path.relpath(T.DIGESTS, ROOT)}")


if __name__ == "__main__":
    main()
