"""Generates tests/golden/reference_configs.json: the reference's argument sets as its loader builds them - configs/base.yaml
overlaid with each dataset's base file along the `parent:` chain - read from the reference tree (oracle/ref_shim.py)
with PyYAML.  Build container only; the values are committed so tests/test_mapping_cpu.py can check replica_args() /
tum_args() / scannetpp_args() anywhere.

    python oracle/gen_config_golden.py
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.ref_shim import REF  # noqa: E402
LEAVES = ("replica_base.yaml", "tum_base.yaml", "scannetpp_base.yaml")


def load(path):
    import yaml
    d = yaml.safe_load(open(path))
    parent = d.pop("parent", None)
    base = load(os.path.join(REF, parent)) if parent not in (None, "None", "") else {}
    base.update(d)
    return base


def main():
    out = {leaf: load(os.path.join(REF, "configs", leaf)) for leaf in LEAVES}
    with open(os.path.join(ROOT, "tests", "golden", "reference_configs.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
