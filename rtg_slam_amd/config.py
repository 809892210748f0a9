"""The reference's config loader (utils/config_utils.py:read_config) on top of this package's argument presets.

    load_config(path)  the YAML chain along `parent:` (shallow dict.update, the child wins; leading `_` stripped from keys;
                       the chain ends at `parent: "None"`), overlaid on the preset of the config's `type`
                       (mapping.replica_args / tum_args / scannetpp_args; `Ours` uses the Replica preset), as a SimpleNamespace

Where a parent lives: the reference opens `parent` relative to the working directory and silently stops the chain when the
file is not there.  Here the working directory is tried first too; then the path relative to each ancestor of the
directory of the file that names the parent, so `configs/replica/office0.yaml` finds `configs/replica_base.yaml` from any
working directory.  A parent found nowhere is an error, not the end of the chain."""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Dict, List, Tuple

from . import mapping as mp

PRESETS = {"Replica": mp.replica_args, "TUM": mp.tum_args, "Scannetpp": mp.scannetpp_args, "Ours": mp.replica_args}


def _read_yaml(path: str) -> Dict:
    import yaml
    with open(path, "r") as f:
        d = yaml.safe_load(f)
    if not isinstance(d, dict):
        raise ValueError(f"rtg_slam_amd.config: {path} is not a YAML mapping")
    return d


def _ends(parent) -> bool:
    return parent is None or parent == "None"


def find_parent(parent: str, child_path: str) -> str:
    """`parent` as the reference opens it (relative to the working directory), else relative to each ancestor of the
    directory of `child_path`, nearest first.  Raises FileNotFoundError when no candidate exists."""
    if os.path.isfile(parent):
        return parent
    tried = [os.path.abspath(parent)]
    d = os.path.dirname(os.path.abspath(child_path))
    while True:
        cand = os.path.join(d, parent)
        tried.append(cand)
        if os.path.isfile(cand):
            return cand
        up = os.path.dirname(d)
        if up == d:
            break
        d = up
    raise FileNotFoundError(f"rtg_slam_amd.config: parent {parent!r} of {child_path} not found; tried " + ", ".join(tried))


def read_chain(config_path: str) -> Tuple[Dict, List[str]]:
    """read_config's merge (config_utils.py:21-34) with the parent lookup above -> (merged dict with keys as written and
    `parent` = the last file's parent, i.e. "None"; the files read, leaf first)."""
    merged = _read_yaml(config_path)
    files = [config_path]
    seen = {os.path.realpath(config_path)}
    cur = config_path
    while not _ends(merged.get("parent")):
        path = find_parent(str(merged["parent"]), cur)
        if os.path.realpath(path) in seen:
            raise ValueError(f"rtg_slam_amd.config: parent cycle at {path}")
        seen.add(os.path.realpath(path))
        parent = _read_yaml(path)
        grand = parent.get("parent")
        parent.update(merged)
        merged = parent
        merged["parent"] = grand
        files.append(path)
        cur = path
    return merged, files


def load_config(config_path: str) -> SimpleNamespace:
    """The argument set of a reference config file: the preset of its `type`, then every key of the YAML chain (leading
    `_` stripped).  Keys this package reads that the chain lacks keep their preset values."""
    merged, files = read_chain(config_path)
    typ = merged.get("type", "Replica")
    if typ not in PRESETS:
        raise ValueError(f"rtg_slam_amd.config: unknown dataset type {typ!r} in {config_path} (known: {sorted(PRESETS)})")
    args = PRESETS[typ]()
    for k, v in merged.items():
        setattr(args, str(k).lstrip("_"), v)
    args.config_files = files
    return args
