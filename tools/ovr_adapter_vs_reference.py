"""Development-time check: the OVR-facing half of ovr_plugin/device_nnvolume_amd.cpp is not compiled here (OVR's headers are not in the
image); every identifier it uses that is not this library's own must at least occur in the reference's own plugin sources (device/), so that
a member name cannot be a typo nobody's compiler has seen.  Which of the adapter's identifiers occur there is read from
tests/golden/reference_ovr_identifiers.json, which `--record REFERENCE_DIR` writes from a checkout of the reference; an identifier the
adapter took up after that recording counts as unknown until it is recorded again.
usage: python tools/ovr_adapter_vs_reference.py [--record REFERENCE_DIR]"""
import glob
import json
import os
import re
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_ovr_identifiers.json")
RECORD = len(sys.argv) == 3 and sys.argv[1] == "--record"
if len(sys.argv) != 1 and not RECORD:
    sys.exit(__doc__)
mine = open(os.path.join(ROOT, "ovr_plugin", "device_nnvolume_amd.cpp")).read()
code = mine[mine.index("#if defined(VNR_HAVE_OVR)"):]
code = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", code, flags=re.S))
code = re.sub(r'"[^"\n]*"', " ", code)
KEYWORDS = set("""if else for while return const auto int float double bool void size_t uint32_t uint8_t char static inline struct class public private
override namespace using typedef new delete this nullptr true false std string vector shared_ptr make_shared runtime_error throw try catch unsigned long sizeof
defined endif include define ifdef ifndef""".split())
OWN = {"bytes", "dev_", "device_nnvolume_amd"}   # this file's locals
ids = sorted({i for i in re.findall(r"[A-Za-z_]\w*(?:::[A-Za-z_]\w*)*", code)
              if i not in KEYWORDS and len(i) > 2 and not i.startswith(("vnrAmd", "vnr_amd", "VNR_", "std::"))})
if RECORD:
    ref = "".join(open(f, errors="ignore").read() for f in glob.glob(os.path.join(sys.argv[2], "device", "*")) if os.path.isfile(f))
    found = sorted({i.split("::")[-1] for i in ids if i.split("::")[-1] in ref})
    with open(GOLDEN, "w") as f:
        json.dump({"what": "the identifiers of the OVR-facing half of ovr_plugin/device_nnvolume_amd.cpp that occur in the reference's device/ "
                           "sources; written by tools/ovr_adapter_vs_reference.py --record", "found": found}, f, indent=1)
        f.write("\n")
    print(f"recorded {len(found)} identifiers in {os.path.relpath(GOLDEN, ROOT)}")
    sys.exit(0)
found = set(json.load(open(GOLDEN))["found"])
unknown = [i for i in ids if i not in OWN and i.split("::")[-1] not in found]
print(f"{len(ids)} identifiers in the OVR-facing half; {len(ids) - len(unknown)} occur in the reference's device/ sources or are this file's own" + (f"; unknown: {unknown}" if unknown else ""))
sys.exit(1 if unknown else 0)
