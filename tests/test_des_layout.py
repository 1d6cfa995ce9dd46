"""CPU check of the DES workspaces (csrc/des_layout.h, DESIGN.md §10.6 and
§10.9): tests/cpp/des_layout_check.cpp runs both engines' layout functions
over the product's plan (build_des_plan) of a graph and over a grid of
item-engine sizes, and checks that sizing and carving agree and that the parts
are aligned, inside the allocation, large enough and disjoint.  Built twice:
plain, and with the address and undefined-behaviour sanitizers.

The sizes it prints are pinned to the values of the commit before the layout
functions existed: printed then by a scratch program (not kept) that evaluated
that commit's byte formulas (des_workspace_bytes, des_items_workspace_bytes)
on the same plans, with the same stand-ins for rocPRIM's temporary sizes
(radix sort 4096 bytes, u64 scan 1024 bytes)."""
import json
import os
import shutil
import subprocess

import pytest

from isim.yamljson import obj_to_json, yaml_to_json

from conftest import TOPOLOGIES
from test_des_gpu import _sleepy_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "istio-isotope_amd", "csrc")


def _canonical_cyclic():
    doc = json.loads(yaml_to_json(open(os.path.join(TOPOLOGIES, "canonical.yaml"), "rb").read()))
    for s in doc["services"]:
        s["script"] = [{"sleep": "250us"}] + s.get("script", [])
    return doc


GRAPHS = {
    "leaf_replicas_tree": lambda: _sleepy_tree(3, 4, reps_leaves=3),
    "canonical_cyclic": _canonical_cyclic,  # a cyclic schedule with step begins and the sort path
    "one_service": lambda: {"services": [{"name": "a", "isEntrypoint": True, "errorRate": 0.2,
                                          "script": [{"sleep": "1ms"}]}]},
}
# isim_des_workspace_bytes of the static engine per n (1, 255, 256, 4097, 5000)
STATIC_BYTES = {
    "leaf_replicas_tree": [23552, 106496, 106496, 1460480, 1773568],
    "canonical_cyclic": [13568, 58112, 58112, 786944, 955648],
    "one_service": [4864, 11008, 11008, 120064, 145152],
}
# and of the item engine (per trace only) per n (1, 255, 256, 3000, 4097, 5000)
ITEMS_BYTES = [2816, 10752, 10752, 109824, 150272, 182528]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("dlc") / "des_layout_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "des_layout_check.cpp")] + \
        [os.path.join(CSRC, f) for f in ("json.cpp", "gounits.cpp", "graph.cpp", "program.cpp", "des_plan.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san, "-I", os.path.join(ROOT, "include"), "-I", CSRC, *srcs,
                    "-o", out], check=True)
    return out


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_layouts(checker, tmp_path, name):
    (tmp_path / "g.json").write_text(obj_to_json(GRAPHS[name]()))
    r = subprocess.run([checker, str(tmp_path / "g.json")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = r.stdout.split("\n")
    assert "layouts ok" in lines
    got = lambda kind: [int(ln.split("bytes=")[1]) for ln in lines if ln.startswith(kind + " n=")]
    assert got("static") == STATIC_BYTES[name]
    assert got("items") == ITEMS_BYTES
