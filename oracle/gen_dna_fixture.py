#!/usr/bin/env python3
"""Generate tests/golden/dna_fixture.json: the parts of Reef's DNA test data that tests/test_safa_shape.py checks the BRCA literals
against, so that the test runs on a checkout alone.  Kept: the lines of tests/scripts/dna.sh that carry the regexes, and of each
1 MB document its length, its SHA-256 and the 10 000 characters appended to the 1 000 000-character base (where the literals sit).

    python oracle/gen_dna_fixture.py <Reef's tests/ directory>
"""
import hashlib
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "dna_fixture.json")
SCRIPT_LINES = (6, 7, 8, 11, 13)           # dna.sh, 1-based
DOCS = ("BRCA1_base1m+primary", "BRCA2_base1m+primary")
BASE = 1000000


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    tests_dir = sys.argv[1]
    with open(os.path.join(tests_dir, "scripts", "dna.sh")) as f:
        sh = f.read().splitlines()
    out = {"generated_by": "oracle/gen_dna_fixture.py from Reef's tests/scripts/dna.sh and tests/docs/",
           "dna_sh": {str(i): sh[i - 1] for i in SCRIPT_LINES}, "docs": {}}
    for name in DOCS:
        with open(os.path.join(tests_dir, "docs", name), "rb") as f:
            doc = f.read()
        out["docs"][name] = {"length": len(doc), "sha256": hashlib.sha256(doc).hexdigest(), "tail_offset": BASE,
                             "tail": doc[BASE:].decode("ascii")}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
