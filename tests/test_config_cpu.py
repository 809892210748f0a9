"""rtg_slam_amd.config: the reference's read_config (utils/config_utils.py) on the committed settings-only copies of its
YAML files (tests/golden/configs), against the argument sets its loader builds (tests/golden/reference_configs.json)."""
import json
import os

import pytest

from rtg_slam_amd import config, mapping as mp

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = os.path.join(HERE, "golden", "configs")
GOLDEN = json.load(open(os.path.join(HERE, "golden", "reference_configs.json")))


def _yaml(path):
    import yaml
    return yaml.safe_load(open(path))


@pytest.mark.parametrize("leaf, base, preset", [("replica/office0.yaml", "replica_base.yaml", mp.replica_args),
                                                ("tum/fr1_desk.yaml", "tum_base.yaml", mp.tum_args)])
def test_leaf_is_its_base_overlaid_with_its_own_keys(leaf, base, preset, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                      # the parents ("configs/...") resolve through the ancestor lookup
    args = config.load_config(os.path.join(CFG, leaf))
    want = dict(GOLDEN[base])
    own = _yaml(os.path.join(CFG, leaf))
    own.pop("parent")
    want.update(own)
    for k, v in want.items():
        assert getattr(args, k) == v, k
    assert args.parent == "None"                     # as read_config leaves it: the last file's parent
    for k in vars(preset()):                         # every key the package reads is there
        assert hasattr(args, k), k


@pytest.mark.parametrize("base", ["replica_base.yaml", "tum_base.yaml", "scannetpp_base.yaml"])
def test_base_files_reproduce_the_reference_loader(base, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    args = config.load_config(os.path.join(CFG, base))
    for k, v in GOLDEN[base].items():
        assert getattr(args, k) == v, (base, k)
    assert args.type == GOLDEN[base]["type"]


def test_parent_relative_to_the_working_directory_comes_first(tmp_path, monkeypatch):
    (tmp_path / "configs").mkdir()
    (tmp_path / "configs" / "p.yaml").write_text("parent: None\nx: 1\ny: 1\n")
    (tmp_path / "sub").mkdir()
    (tmp_path / "sub" / "configs").mkdir()
    (tmp_path / "sub" / "configs" / "p.yaml").write_text("parent: None\nx: 2\ny: 2\n")
    (tmp_path / "sub" / "leaf.yaml").write_text("parent: configs/p.yaml\ny: 3\n")
    monkeypatch.chdir(tmp_path)
    a = config.load_config(str(tmp_path / "sub" / "leaf.yaml"))
    assert (a.x, a.y) == (1, 3)                      # the CWD's configs/p.yaml, not the one next to the leaf
    monkeypatch.chdir(tmp_path / "sub" / "configs")
    a = config.load_config(str(tmp_path / "sub" / "leaf.yaml"))
    assert (a.x, a.y) == (2, 3)                      # nearest ancestor of the leaf's directory


def test_missing_parent_raises(tmp_path, monkeypatch):
    (tmp_path / "leaf.yaml").write_text("parent: configs/nowhere.yaml\nx: 1\n")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="nowhere"):
        config.load_config(str(tmp_path / "leaf.yaml"))


def test_underscore_keys_child_wins_and_type_preset(tmp_path, monkeypatch):
    (tmp_path / "configs").mkdir()
    (tmp_path / "configs" / "b.yaml").write_text("parent: None\ntype: TUM\n_hidden: 5\nmemory_length: 9\nz: [1, 2]\n")
    (tmp_path / "configs" / "l.yaml").write_text("parent: configs/b.yaml\nmemory_length: 7\n__two: x\n")
    monkeypatch.chdir(tmp_path / "configs")
    a = config.load_config("l.yaml")
    assert a.hidden == 5 and a.two == "x" and not hasattr(a, "_hidden")
    assert a.memory_length == 7 and a.z == [1, 2]
    assert a.stable_confidence_thres == mp.tum_args().stable_confidence_thres        # not in the chain: the TUM preset
    (tmp_path / "configs" / "o.yaml").write_text("parent: None\ntype: Ours\n")
    o = config.load_config(str(tmp_path / "configs" / "o.yaml"))
    assert o.type == "Ours" and o.uniform_sample_num == mp.replica_args().uniform_sample_num
    (tmp_path / "configs" / "u.yaml").write_text("parent: None\ntype: Blender\n")
    with pytest.raises(ValueError, match="Blender"):
        config.load_config(str(tmp_path / "configs" / "u.yaml"))
