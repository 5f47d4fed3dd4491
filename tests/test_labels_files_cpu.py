"""The file-level side of the label geometry without a GPU: `degrade_files` and `python -m edtr_amd.degrade` take the new keywords and
flags and keep their defaults, and a geometry file is read with the reference's keys.  What the launches write is checked on the device
by tests/test_gpu_labels_files.py."""
import inspect

import pytest

from edtr_amd import degrade, labels


def test_degrade_files_takes_geometry_and_masks_and_defaults_to_neither():
    sig = inspect.signature(degrade.degrade_files)
    assert sig.parameters["geometry"].default is None and sig.parameters["masks"].default is None
    assert list(sig.parameters)[:7] == ["paths", "out_dir", "cfg", "seed", "batch_size", "workers", "device"]      # the existing order stands


def test_command_line_flags():
    ap = degrade.build_parser()
    base = ["--input", "in", "--output", "out", "--config", "codeformer", "--seed", "3"]
    args = ap.parse_args(base)
    assert args.geometry is None and args.masks is None
    args = ap.parse_args(base + ["--geometry", "geo.yaml", "--masks", "SegmentationClass"])
    assert args.geometry == "geo.yaml" and args.masks == "SegmentationClass"


def test_geometry_is_read_from_a_yaml_file_with_the_references_keys(tmp_path):
    path = tmp_path / "geo.yaml"
    path.write_text("dataset:\n  train:\n    target: datasets.segmentation.DegradedSegmentationDataset\n    params:\n      root: somewhere\n"
                    "      gt_size: 560\n      resize_range: [0.5, 2.0]\n      out_size: 512\n      crop_type: random\n      hflip: true\n"
                    "      rotation: false\n      blur_kernel_size: 41\n")
    cfg = labels.load_geometry(str(path))
    assert (cfg.gt_size, list(cfg.resize_range), cfg.out_size, cfg.crop_type, cfg.hflip) == (560, [0.5, 2.0], 512, "random", True)
    assert labels.load_geometry(cfg) is cfg
    assert labels.load_geometry({"gt_size": 32, "out_size": 24}).out_size == 24
    path.write_text("gt_size: 64\nrotation: true\n")
    with pytest.raises(NotImplementedError):
        labels.load_geometry(str(path))
