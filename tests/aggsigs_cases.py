"""The inputs the CPU and GPU tests of the per-group signature aggregation share: tests/golden/aggregate_signatures.json
(tests/golden/gen_aggregate_signatures.py) laid out as the calls take it, and the signature encodings of tests/golden/deser_adversarial.json."""
import deser_cases as dc
from util import golden

INF192, INF96 = bytes(192), bytes([0xc0]) + bytes(95)


def fixture():
    return golden("aggregate_signatures")


def table_of(fx):
    t = bytes.fromhex(fx["table"])
    return [t[192 * i:192 * i + 192] for i in range(len(t) // 192)]


def contiguous_inputs(fx=None):
    """-> (signatures laid end to end, offsets, expected 192-byte images, expected 96-byte wire forms, expected status bytes)"""
    fx = fx or fixture()
    tab = table_of(fx)
    sigs = b"".join(tab[i] for g in fx["groups"] for i in g["members"])
    offsets = [0]
    for g in fx["groups"]:
        offsets.append(offsets[-1] + len(g["members"]))
    return (sigs, offsets, b"".join(bytes.fromhex(g["out192"]) for g in fx["groups"]), b"".join(bytes.fromhex(g["out96"]) for g in fx["groups"]),
            bytes(g["status"] for g in fx["groups"]))


def indexed_inputs(bad=False, fx=None):
    """-> (table, idx, offsets, expected images, wire forms, status bytes) of the indexed form; bad: with the out-of-range index in place"""
    fx = fx or fixture()
    ix = fx["indexed"]
    _, _, w192, w96, status = contiguous_inputs(fx)
    idx = list(ix["idx"])
    if bad:
        b = ix["bad_index"]
        idx[b["position"]] = b["value"]
        g = b["group"]
        w192 = w192[:192 * g] + INF192 + w192[192 * g + 192:]
        w96 = w96[:96 * g] + INF96 + w96[96 * g + 96:]
        status = status[:g] + bytes([b["status"]]) + status[g + 1:]
    return bytes.fromhex(fx["table"]), idx, list(ix["offsets"]), w192, w96, status


def adversarial_signatures(unc):
    """[(name, wire bytes)] of every signature encoding the adversarial rows use that has this wire form (deser_cases.wire), in fixture order"""
    fx = dc.fixture()
    names = []
    for r in fx["rows"]:
        if r["sig"] not in names:
            names.append(r["sig"])
    out = []
    for nm in names:
        b = dc.wire(fx["enc"][nm], "sig", unc)
        if b is not None:
            out.append((nm, b))
    return out
