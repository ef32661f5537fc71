#!/usr/bin/env python3
"""Generates tests/golden/visualize_golden.npz by RUNNING THE REFERENCE: `write_ply`, `write_bbox` and the `visualize` loops of
scripts/visualize_grounding.py and scripts/visualize_captioning.py.  The two scripts cannot be imported (they list a directory that
does not exist and import plyfile at import time), so the function definitions are taken out of the parsed module with `ast` and
executed with numpy; `load_data` returns the canned case, OUTPUT_ROOT is a temporary directory, tqdm is the identity and
`visualize_aligned_mesh` does nothing (mesh.ply needs plyfile and a scan; it is not part of the golden).  Nothing of the reference's
text is stored.  Run in the build container only (needs /root/reference); the tests never run it.

Inputs are not stored: tests/visualize_restate.py's `box_cases`, `grounding_tree_case` and `captioning_tree_case` rebuild them.
Stored: the complete bytes of every file the reference wrote, under "box/<case>", "ground/<relative path>", "cap/<relative path>"."""
import ast
import math
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import visualize_restate as VR  # noqa: E402


def reference_functions(script, names, **replaced):
    """the named top-level functions of a reference script, compiled from its own source into a namespace of our making"""
    path = os.path.join(REF, "scripts", script)
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), (script, [n.name for n in body])
    ns = {"np": np, "os": os, "math": math, "tqdm": lambda it: it}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    ns.update(replaced)
    return ns


def tree_files(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def main():
    files = {}
    with tempfile.TemporaryDirectory() as tmp:
        ground = reference_functions("visualize_grounding.py", ("write_ply", "write_bbox", "visualize"), OUTPUT_ROOT=tmp,
                                     load_data=lambda args: VR.grounding_tree_case(), visualize_aligned_mesh=lambda *a: None)
        cap = reference_functions("visualize_captioning.py", ("write_ply", "write_bbox", "visualize"), OUTPUT_ROOT=tmp,
                                  load_data=lambda args: VR.captioning_tree_case()[0], visualize_aligned_mesh=lambda *a: None)
        for i, (name, corners, mode) in enumerate(VR.box_cases()):
            # the two scripts carry the same write_bbox: alternate between them
            path = os.path.join(tmp, name + ".ply")
            (ground if i % 2 == 0 else cap)["write_bbox"](corners.copy(), mode, path)
            files["box/" + name] = open(path, "rb").read()
        args = types.SimpleNamespace(folder="run")
        ground["visualize"](args)
        for rel, data in tree_files(os.path.join(tmp, "run", "vis_grounding")).items():
            files["ground/" + rel] = data
        cap["visualize"](args)
        for rel, data in tree_files(os.path.join(tmp, "run", "vis_captioning")).items():
            files["cap/" + rel] = data
    names = sorted(files)
    arrays = {"file%03d" % i: np.frombuffer(files[n], np.uint8) for i, n in enumerate(names)}
    out = os.path.join(HERE, "visualize_golden.npz")
    np.savez_compressed(out, names=np.array(names), **arrays)
    print("wrote %s: %d files, %d bytes of text, %d bytes on disk" % (out, len(names), sum(len(v) for v in files.values()), os.path.getsize(out)))


if __name__ == "__main__":
    main()
