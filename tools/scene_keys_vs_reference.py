"""Development-time check: every JSON key and enumeration string the reference's scene reader (serializer.cpp) mentions is a string of this
library's reader (csrc/scene.cpp) too, or is listed below with the reason it is not.  The reference's strings are read from
tests/golden/reference_scene_keys.json, which `--record REFERENCE_DIR` writes from a checkout of the reference.
usage: python tools/scene_keys_vs_reference.py [--record REFERENCE_DIR]"""
import json
import os
import re
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_scene_keys.json")


def literals(path):
    t = open(path).read()
    t = re.sub(r"/\*.*?\*/", " ", t, flags=re.S)
    t = re.sub(r"//[^\n]*", " ", t)
    return set(re.findall(r'"([A-Za-z_][\w .\-]*)"', t))


NOT_HERE = {
    "serializer.h": "an include",
    "fileUpperLeft": "read into a local the reference never uses (serializer.cpp:274, 301)",
    "LITTLE_ENDIAN": "the default; this reader tests for BIG_ENDIAN only, any other string is little endian there as here (enum mapping, :36-40)",
    "transferFunction": "decoded by OVR's tfn module, absent from the tree: the shim hands the node to the application's decoder (vnr_api_shim.hpp)",
}
if len(sys.argv) == 3 and sys.argv[1] == "--record":
    keys = sorted(literals(os.path.join(sys.argv[2], "serializer.cpp")))
    with open(GOLDEN, "w") as f:
        json.dump({"what": "the string literals of the reference's serializer.cpp (JSON keys, enumeration strings); written by "
                           "tools/scene_keys_vs_reference.py --record", "strings": keys}, f, indent=1)
        f.write("\n")
    print(f"recorded {len(keys)} strings in {os.path.relpath(GOLDEN, ROOT)}")
    sys.exit(0)
if len(sys.argv) != 1:
    sys.exit(__doc__)
ref, mine = set(json.load(open(GOLDEN))["strings"]), literals(os.path.join(ROOT, "instantvnr_amd", "csrc", "scene.cpp"))
unexplained = sorted(k for k in ref - mine if k not in NOT_HERE)
print(f"{len(ref)} strings in the reference's reader, {len(ref & mine)} of them here, {len(ref - mine) - len(unexplained)} explained:")
for k in sorted(ref - mine):
    print(f"   {k}: {NOT_HERE.get(k, 'UNEXPLAINED')}")
sys.exit(1 if unexplained else 0)
