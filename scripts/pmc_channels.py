"""Per-instance values of ONE counter from a rocprofv3 --pmc <counter> --output-format json run, per kernel.

    python3 scripts/pmc_channels.py <results.json> [name filter]

A TCC counter has one instance per (XCD, L2 channel).  Per kernel (summed over its dispatches): the number of instances, how
many of them counted anything, max / mean over the instances, and the values themselves in instance order -- the skew of
the L2 channels under that kernel.  The instance is the record's id as the file gives it (counter and dimensions packed in
one integer) or, where the records of a dispatch carry the counter's id alone, the record's position in the dispatch's list:
the tool writes them in the order of the counter's `instances` table (XCD-major, 16 channels per XCD on gfx950).
"""
import collections
import json
import sys


def walk(node, found):
    """every dict that looks like a dispatch's counter record set: has 'records' (list) next to dispatch data"""
    if isinstance(node, dict):
        if isinstance(node.get("records"), list) and ("dispatch_data" in node or "dispatch_info" in node):
            found.append(node)
        for v in node.values():
            walk(v, found)
    elif isinstance(node, list):
        for v in node:
            walk(v, found)


def find_key(node, key):
    if isinstance(node, dict):
        if key in node:
            return node[key]
        for v in node.values():
            r = find_key(v, key)
            if r is not None:
                return r
    elif isinstance(node, list):
        for v in node:
            r = find_key(v, key)
            if r is not None:
                return r
    return None


def handle(x):
    return x.get("handle", x.get("value")) if isinstance(x, dict) else x


def main():
    doc = json.load(open(sys.argv[1]))
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    names = {}
    syms = find_key(doc, "kernel_symbols") or []
    for s in syms:
        if isinstance(s, dict) and "kernel_id" in s:
            n = s.get("formatted_kernel_name") or s.get("truncated_kernel_name") or s.get("kernel_name") or ""
            names[s["kernel_id"]] = n.replace("void ", "").replace("msda::(anonymous namespace)::", "")
    sets = []
    walk(doc, sets)
    acc = collections.OrderedDict()
    calls = collections.Counter()
    for cs in sets:
        kid = find_key(cs.get("dispatch_data", cs), "kernel_id")
        name = str(names.get(kid, kid))
        if flt and flt not in name:
            continue
        calls[name] += 1
        d = acc.setdefault(name, collections.defaultdict(float))
        for pos, r in enumerate(cs["records"]):
            inst = (handle(r.get("id", r.get("counter_id"))), pos if "id" not in r else 0)
            d[inst] += float(r.get("value", r.get("counter_value", 0.0)))
    if not sets:
        print("no counter records found; top-level keys:", list(doc.keys()) if isinstance(doc, dict) else type(doc))
    for name, d in acc.items():
        vals = [d[k] for k in sorted(d)]
        mean = sum(vals) / max(len(vals), 1)
        print("%s  calls %d" % (name[:70], calls[name]))
        print("   instances %d  non-zero %d  total %.0f  max/mean %.3f  min/mean %.3f" %
              (len(vals), sum(1 for v in vals if v > 0), sum(vals), max(vals) / mean if mean else 0.0, min(vals) / mean if mean else 0.0))
        per = [v / calls[name] for v in vals]
        for i in range(0, len(per), 16):
            print("   " + " ".join("%8.0f" % v for v in per[i:i + 16]))


if __name__ == "__main__":
    main()
