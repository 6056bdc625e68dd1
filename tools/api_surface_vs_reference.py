"""Development-time check: every function the reference's api.h declares, by name, number of parameters and the parameters' types
(namespace prefixes, parameter names, defaults and white space dropped), is defined by include/vnr_api_shim.hpp with the same list, and its
enumerations have the same enumerators in the same order.  The reference's side is read from tests/golden/reference_api_surface.json, which
`--record` extracts from a checkout of the reference (its api.h), so that the check needs nothing outside this repository.
usage: python tools/api_surface_vs_reference.py [--record REFERENCE_DIR]"""
import json
import os
import re
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_api_surface.json")


def strip(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def split_params(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "<(":
            depth += 1
        if ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur); cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    return out


def ptype(p):
    p = p.split("=")[0].strip()
    p = re.sub(r"\b(vnr|std)::", "", p)
    # drop a trailing parameter name (an identifier after the type), keep pointers / references
    m = re.match(r"^(.*?[\w>\*&])\s+(\w+)$", p)
    if m and m.group(2) not in ("int", "float", "double", "bool", "char", "size_t", "uint8_t"):
        p = m.group(1)
    return re.sub(r"\s+", "", p)


RETURNS = {}


def signatures(text, definitions):
    sigs = set()
    pat = r"([\w:<>\*&]+(?:\s*[\*&])?)\s+(vnr[A-Z]\w*)\s*\(([^()]*(?:\([^()]*\)[^()]*)*)\)\s*" + (r"\{" if definitions else r";")
    for m in re.finditer(pat, strip(text)):
        sig = (m.group(2), tuple(ptype(p) for p in split_params(m.group(3))))
        sigs.add(sig)
        RETURNS[(definitions, sig)] = re.sub(r"\b(vnr|std)::", "", m.group(1)).replace(" ", "")
    return sigs


# the enumerations of api.h (rendering modes, value types): the same enumerators in the same order
def enums(text):
    out = {}
    for m in re.finditer(r"\benum\s+(?:class\s+)?(\w+)\s*(?::\s*\w+\s*)?\{([^}]*)\}", strip(text)):
        out[m.group(1)] = [e.split("=")[0].strip() for e in m.group(2).split(",") if e.strip()]
    return out


if len(sys.argv) == 3 and sys.argv[1] == "--record":
    text = open(os.path.join(sys.argv[2], "api.h")).read()
    sigs = signatures(text, False)
    doc = {"what": "the reference's api.h as this check reads it: each declaration's name, parameter types and return type (namespace prefixes, "
                   "parameter names and defaults dropped), and each enumeration's enumerators; written by tools/api_surface_vs_reference.py --record",
           "functions": [{"name": n, "params": list(p), "returns": RETURNS[(False, (n, p))]} for n, p in sorted(sigs)],
           "enums": enums(text)}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"recorded {len(sigs)} declarations and {len(doc['enums'])} enumerations in {os.path.relpath(GOLDEN, ROOT)}")
    sys.exit(0)
if len(sys.argv) != 1:
    sys.exit(__doc__)
golden = json.load(open(GOLDEN))
ref = set()
for fn in golden["functions"]:
    s = (fn["name"], tuple(fn["params"]))
    ref.add(s)
    RETURNS[(False, s)] = fn["returns"]
shim = signatures(open(os.path.join(ROOT, "include", "vnr_api_shim.hpp")).read(), True)
missing = sorted(s for s in ref if s not in shim)
by_arity = {(n, len(p)) for n, p in shim}
print(f"api.h declares {len(ref)} functions ({len({n for n, _ in ref})} names); the shim defines {len(shim)}")
for n, p in missing:
    print(("   same name and number of parameters, types written differently: " if (n, len(p)) in by_arity else "   MISSING: ") + n + "(" + ", ".join(p) + ")")
hard = [s for s in missing if (s[0], len(s[1])) not in by_arity]
ret_diff = [(s, RETURNS[(False, s)], RETURNS[(True, s)]) for s in sorted(ref) if s in shim and RETURNS[(False, s)] != RETURNS[(True, s)]]
for s_, a, b in ret_diff:
    print(f"   return type of {s_[0]}: {a} there, {b} here")
print(f"{len(ref) - len(missing) - len(ret_diff)} of {len(ref)} declarations have the same return type too")
hard += ret_diff
print(f"{len(ref) - len(missing)} of {len(ref)} declarations have a definition with the same parameter types; {len(hard)} have none with that name and arity")


ref_e, shim_e = golden["enums"], enums(open(os.path.join(ROOT, "include", "vnr_api_shim.hpp")).read())
for name, items in ref_e.items():
    ok = shim_e.get(name) == items
    hard += [] if ok else [name]
    print(f"{'ok ' if ok else 'BAD'} enum {name}: {len(items)} enumerators" + ("" if ok else f"; here {shim_e.get(name)}"))
sys.exit(1 if hard else 0)
