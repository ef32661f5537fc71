#!/usr/bin/env python3
"""Generates tests/golden/scan_export_golden.npz by RUNNING THE REFERENCE's own scan export: data/scannet/prepare_scannet.py
(export, process_one_scan) and the main body of prepare_scannet_inst_gt.py, on small synthetic scans from tests/scan_synth.py.
`plyfile.PlyData` is a stub that serves the very structured arrays the synthetic writer put into the files (plyfile is not needed);
`omegaconf.OmegaConf` is a namespace stub, `tqdm` the identity.  Stores each scan's raw file bytes and the reference's outputs.
Run where the reference is available."""
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import scan_synth as SS  # noqa: E402

REF = "/root/reference"
CASES = [("scene0000_00", dict(seed=11, n=2400, n_objects=14)),
         ("scene0217_00", dict(seed=12, n=1800, n_objects=12)),
         ("scene0001_00", dict(seed=13, n=1500, n_objects=10, align=False, empty_object=True))]

_ARRAYS = {}   # file path -> {element: structured array}


class _Element:
    def __init__(self, data):
        self.data, self.count = data, len(data)

    def __getitem__(self, k):
        return self.data[k]


class _PlyData:
    def __init__(self, els):
        self.els = els

    @staticmethod
    def read(f):
        return _PlyData(_ARRAYS[os.path.abspath(f.name)])

    def __getitem__(self, k):
        return _Element(self.els[k])


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def main():
    _stub("plyfile", PlyData=_PlyData, PlyElement=None)
    cfg_holder = {}
    _stub("omegaconf", OmegaConf=_ns(load=lambda path: cfg_holder["cfg"]))
    _stub("tqdm", tqdm=lambda x: x)
    sys.path.insert(0, os.path.join(REF, "data", "scannet"))
    import prepare_scannet as PS
    load = torch.load
    torch.load = lambda f, *a, **k: load(f, *a, **dict(k, weights_only=False))   # the reference's pickled numpy arrays
    out = {"cases": np.array([c for c, _ in CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        cfg = _ns(SCANNETV2_PATH=_ns(raw_scans=os.path.join(tmp, "scans"), split_data=os.path.join(tmp, "split"),
                                     split_gt=os.path.join(tmp, "gt")), split="val")
        cfg_holder["cfg"] = cfg
        os.makedirs(os.path.join(tmp, "split", "val"))
        for scene, kw in CASES:
            scan = SS.make_scan(**kw)
            files = SS.scan_files(scene, scan)
            d = SS.write_files(os.path.join(tmp, "scans", scene), files)
            v = np.zeros(len(scan["vertex"]), SS.LABEL_VERTEX_DTYPE)
            for k in SS.VERTEX_DTYPE.names:
                v[k] = scan["vertex"][k]
            v["label"] = scan["labels"]
            face = np.zeros(len(scan["faces"]), [("vertex_indices", "<i4", (3,))])
            face["vertex_indices"] = scan["faces"]
            _ARRAYS[os.path.abspath(os.path.join(d, scene + "_vh_clean_2.ply"))] = {"vertex": scan["vertex"], "face": face}
            _ARRAYS[os.path.abspath(os.path.join(d, scene + "_vh_clean_2.labels.ply"))] = {"vertex": v, "face": face}
            for name, data in files.items():
                out["%s/file/%s" % (scene, name)] = np.frombuffer(data, np.uint8)
            PS.process_one_scan(scene, cfg)
            r = torch.load(os.path.join(tmp, "split", "val", scene + ".pth"))
            for k, a in r.items():
                out["%s/%s" % (scene, k)] = a
        sys.argv = ["prepare_scannet_inst_gt.py", "-s", "val", "-c", "unused.yaml"]
        runpy.run_path(os.path.join(REF, "data", "scannet", "prepare_scannet_inst_gt.py"), run_name="__main__")
        for scene, _ in CASES:
            out["%s/inst_gt" % scene] = np.loadtxt(os.path.join(tmp, "gt", "val", scene + ".txt"), dtype=np.int64).astype(np.int32)
    path = os.path.join(HERE, "scan_export_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
