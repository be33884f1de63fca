"""The inputs the CPU and GPU tests of the threshold-signature recovery share: tests/golden/recover_signatures.json
(tests/golden/gen_recover_signatures.py) laid out as the calls take it."""
from util import golden

INF192, INF96 = bytes(192), bytes([0xc0]) + bytes(95)
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def fixture():
    return golden("recover_signatures")


def table_of(fx):
    t = bytes.fromhex(fx["table"])
    return [t[192 * i:192 * i + 192] for i in range(len(t) // 192)]


def expected(groups):
    return (b"".join(bytes.fromhex(g["out192"]) for g in groups), b"".join(bytes.fromhex(g["out96"]) for g in groups), bytes(g["status"] for g in groups))


def contiguous_inputs(fx=None, groups=None):
    """-> (shares laid end to end, ids by position, offsets, expected 192-byte images, 96-byte wire forms, status bytes) of `groups` (all)"""
    fx = fx or fixture()
    groups = fx["groups"] if groups is None else groups
    tab = table_of(fx)
    sigs = b"".join(tab[i] for g in groups for i in g["members"])
    ids = b"".join(bytes.fromhex(x) for g in groups for x in g["ids"])
    offsets = [0]
    for g in groups:
        offsets.append(offsets[-1] + len(g["members"]))
    return (sigs, ids, offsets) + expected(groups)


def indexed_inputs(bad=False, fx=None):
    """-> (table, idx, ids by position, offsets, expected images, wire forms, status bytes) of the indexed form; bad: with the out-of-range index"""
    fx = fx or fixture()
    ix = fx["indexed"]
    _, ids, _, w192, w96, status = contiguous_inputs(fx)
    idx = list(ix["idx"])
    if bad:
        b = ix["bad_index"]
        idx[b["position"]] = b["value"]
        g = b["group"]
        w192 = w192[:192 * g] + INF192 + w192[192 * g + 192:]
        w96 = w96[:96 * g] + INF96 + w96[96 * g + 96:]
        status = status[:g] + bytes([b["status"]]) + status[g + 1:]
    return bytes.fromhex(fx["table"]), idx, ids, list(ix["offsets"]), w192, w96, status


def coefficient(ids, i):
    """the Lagrange coefficient at 0 of member i of a group with these ids (integers), blst_recovery.nim:101-118"""
    xs = [x % R for x in ids]
    a, b = 1, xs[i]
    for j, x in enumerate(xs):
        a = a * x % R
        if j != i:
            b = b * (x - xs[i]) % R
    return a * pow(b, R - 2, R) % R
