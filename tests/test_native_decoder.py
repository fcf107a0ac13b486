"""The engine's section decoder (kuberay_amd/_native/json_decode.hpp) against
json.loads: for every stored entry, ``fetch_tree`` must give exactly what
``json.loads`` of the blob ``fetch`` assembles for the same entry gives, equal
by ``==`` and by exact type at every node (bool vs int, int vs float, the sign
of zero, key order), or hand back that blob (bytes) for the caller to parse.

Fallbacks allowed: none for the golden objects, none for the bench's
objects, and none for the seeded random trees, whose generator leaves out by
construction exactly what the decoder lists as unsupported (integers outside
int64, NaN / Infinity, lone surrogates, keys that collide once json.dumps has
made strings of them, nesting past the limit). The hand-made edge cases say
one by one whether they decode or fall back.
"""
import json
import math
import random
from pathlib import Path

import pytest

try:
    from kuberay_amd._native import engine
    from kuberay_amd.kube.native import NativeBackend
except ImportError:
    pytest.skip("native engine not built", allow_module_level=True)

from kuberay_amd.kube.client import InMemoryClient
from kuberay_amd.kube.store import InMemoryApiServer
from kuberay_amd.ops.raycluster import RayClusterReconciler
from kuberay_amd.testing import simple_raycluster
from kuberay_amd.utils import constants as C

GOLDEN = Path(__file__).resolve().parent / "golden"
KEY = ("X", "d", "n")


def assert_same_tree(got, want, path="$"):
    """== plus exact type at every node, key order, and the sign of zero."""
    assert type(got) is type(want), (path, type(got), type(want))
    if type(want) is dict:
        assert list(got) == list(want), path
        for k in want:
            assert type(k) is str
            assert_same_tree(got[k], want[k], f"{path}.{k}")
    elif type(want) is list:
        assert len(got) == len(want), path
        for i, (a, b) in enumerate(zip(got, want)):
            assert_same_tree(a, b, f"{path}[{i}]")
    elif type(want) is float:
        assert got == want and math.copysign(1, got) == math.copysign(1, want), \
            (path, got, want)
    else:
        assert got == want, (path, got, want)


def put_raw(store, text):
    """A "whole" entry holding ``text`` (str or bytes) as it is."""
    store.put(KEY[0], KEY[1], KEY[2], text, "", [], [])


def check_entry(store, key=KEY):
    """Compares the two reads of one entry. Returns True when the decoder
    produced the tree, False when it handed the blob back."""
    blob = store.fetch(*key)
    before = store.stats()
    got = store.fetch_tree(*key)
    after = store.stats()
    assert after["blobs_assembled"] == before["blobs_assembled"] + 1
    assert after["bytes_assembled"] == before["bytes_assembled"] + len(blob)
    if type(got) is bytes:
        assert got == blob
        assert after["decode_fallbacks"] == before["decode_fallbacks"] + 1
        assert after["trees_decoded"] == before["trees_decoded"]
        return False
    assert after["trees_decoded"] == before["trees_decoded"] + 1
    assert after["decode_fallbacks"] == before["decode_fallbacks"]
    assert_same_tree(got, json.loads(blob))
    return True


def store_both_ways(obj):
    """``obj`` written through put_object (None when the encoder declines)
    and through the blob path; yields (how, store)."""
    out = []
    store = engine.NativeStore(16)
    if store.put_object(KEY[0], KEY[1], KEY[2], obj, None) is not None:
        out.append(("sections", store))
    store = engine.NativeStore(16)
    put_raw(store, json.dumps(obj, separators=(",", ":")))
    out.append(("blob", store))
    return out


# -- golden and bench objects: zero fallbacks --------------------------------

def golden_objects():
    out = []
    for path in sorted(GOLDEN.glob("*.json")):
        doc = json.loads(path.read_text())
        out.append((path.name, doc))
        members = doc.values() if isinstance(doc, dict) else doc
        for i, member in enumerate(members):
            if isinstance(member, dict):
                out.append((f"{path.name}[{i}]", member))
    return out


def test_golden_objects_decode_without_fallback():
    objects = golden_objects()
    assert objects
    for label, obj in objects:
        ways = store_both_ways(obj)
        assert [how for how, _ in ways] == ["sections", "blob"], label
        for how, store in ways:
            assert check_entry(store), (label, how)


def _start_pods(server):
    for pod in server.list("Pod"):
        if (pod.get("status") or {}).get("phase") == "Running":
            continue
        is_head = pod["metadata"]["labels"][C.RAY_NODE_TYPE_LABEL_KEY] == "head"
        index = pod["metadata"]["labels"].get(C.RAY_WORKER_REPLICA_INDEX_KEY, "0")
        ip = "10.244.0.1" if is_head else f"10.244.1.{int(index) + 1}"

        def to_running(p, ip=ip):
            p["status"] = {
                "phase": "Running", "podIP": ip,
                "conditions": [{"type": "Ready", "status": "True"}],
                "containerStatuses": [
                    {"name": c["name"], "ready": True, "state": {"running": {}}}
                    for c in p["spec"]["containers"]]}
        server.mutate_status("Pod", "default", pod["metadata"]["name"], to_running)


@pytest.fixture(scope="module")
def bench_server():
    """One bench cluster (bench.py's shape: 3 workers, 1 GPU each) reconciled
    to ready on the native backend."""
    server = InMemoryApiServer(NativeBackend())
    client = InMemoryClient(server)
    reconciler = RayClusterReconciler(client)
    client.create(simple_raycluster("bench-r0-s0-0000", workers=3,
                                    gpus_per_worker=1))
    request = ("default", "bench-r0-s0-0000")
    reconciler.reconcile(request)
    _start_pods(server)
    reconciler.reconcile(request)
    assert server.get("RayCluster", "default",
                      "bench-r0-s0-0000")["status"]["state"] == "ready"
    return server


def test_bench_objects_decode_without_fallback(bench_server):
    store = bench_server._backend._store
    seen = set()
    for kind in ("RayCluster", "Pod", "Service"):
        for obj in bench_server.list(kind):
            name = obj["metadata"]["name"]
            assert check_entry(store, (kind, "default", name)), (kind, name)
            labels = obj["metadata"].get("labels") or {}
            seen.add((kind, labels.get(C.RAY_NODE_TYPE_LABEL_KEY)))
    assert {("RayCluster", None), ("Pod", "head"), ("Pod", "worker")} <= seen
    assert any(kind == "Service" for kind, _ in seen)
    assert store.stats()["decode_fallbacks"] == 0


# -- hand-made edge cases ------------------------------------------------------

def deep(n, leaf="1"):
    return "[" * n + leaf + "]" * n


DECODES, FALLS_BACK = True, False
U = "\\" + "u"  # the two characters that open a JSON unicode escape
RAW_CASES = [
    ('{}', DECODES), ('[]', DECODES), ('{"a":{},"b":[],"c":[{}],"d":{"e":[[]]}}',
                                       DECODES),
    ('{"":"","x":{"":{"":[]}}}', DECODES),
    (r'"\" \\ \/ \b\f\n\r\t"', DECODES),
    (r'{"a\"b\\c\/d\n":"v"}', DECODES),
    ('"' + U + '0000"', DECODES), ('"a' + U + '0000b"', DECODES),
    ('"' + U + '00e9"', DECODES), ('"' + U + '00E9' + U + '20ac"', DECODES),
    ('"' + U + 'd83d' + U + 'de00"', DECODES),
    ('"x' + U + 'D83D' + U + 'DE00y"', DECODES),
    ('{"k' + U + '00e9":"' + U + '0041"}', DECODES),
    (r'"\ud83d"', FALLS_BACK), (r'"\ude00"', FALLS_BACK),
    (r'"\ud83dA"', FALLS_BACK), (r'{"\udc00":1}', FALLS_BACK),
    ('"café € \U0001f600 中文"', DECODES),
    ('{"éè":"ü","k":["\U0001f600"]}', DECODES),
    ('[-9223372036854775808,9223372036854775807,0,-0,-1,10]', DECODES),
    ('9223372036854775808', FALLS_BACK), ('-9223372036854775809', FALLS_BACK),
    ('[1,[2,{"n":123456789012345678901234567890}]]', FALLS_BACK),
    ('[0.1,1e-7,1E+22,5e-324,1.7976931348623157e308,-0.0,0.0,1.0,1e2,'
     '2.5E-3,-1.5e+10,123456789.123456789,0.30000000000000004,1e0]', DECODES),
    ('[1e400]', FALLS_BACK), ('[-1e400]', FALLS_BACK), ('[1e-400]', FALLS_BACK),
    ('[NaN]', FALLS_BACK), ('{"a":Infinity}', FALLS_BACK),
    ('[-Infinity]', FALLS_BACK),
    ('{"a":1,"a":2}', FALLS_BACK), (r'{"a":1,"b":{"c":1,"c":2}}', FALLS_BACK),
    ('[true,false,null,1,1.0,"1"]', DECODES),
    (' { "a" : [ 1 , 2 ] ,\n"b":\t{ } } ', DECODES),
    (deep(128), DECODES), (deep(129), FALLS_BACK),
    (deep(200), FALLS_BACK),
    ('{"a":' * 200 + '1' + '}' * 200, FALLS_BACK),
    ('"plain"', DECODES), ('17', DECODES), ('null', DECODES),
]


@pytest.mark.parametrize("as_bytes", [False, True])
def test_edge_cases_match_or_fall_back(as_bytes):
    for raw, decodes in RAW_CASES:
        store = engine.NativeStore(16)
        put_raw(store, raw.encode("utf-8") if as_bytes else raw)
        # json.loads takes every one of them: the reference exists
        json.loads(store.fetch(*KEY))
        assert check_entry(store) is decodes, raw[:60]


def test_malformed_whole_blob_falls_back_and_raises_as_before():
    backend = NativeBackend()
    backend._store.put("X", "d", "n", '{"a":', "", [], [])
    with pytest.raises(json.JSONDecodeError):
        backend.fetch(("X", "d", "n"))
    backend._store.put("X", "d", "n", b'"\xff"', "", [], [])
    with pytest.raises(UnicodeDecodeError):
        backend.fetch(("X", "d", "n"))
    assert backend.stats()["decode_fallbacks"] == 2


def test_edge_trees_through_the_encoder():
    """Values as the native encoder writes them (raw UTF-8, its own float
    and escape spellings), in all three sections."""
    tree = {
        "kind": "X", "empty": {}, "none": None, "t": True, "f": False,
        "": {"": ""},
        "floats": [0.1, 1e-7, 1e22, 5e-324, 1.7976931348623157e308, -0.0, 0.0,
                   1.0, 100.0, 1e16, 1e-5, 123456.789],
        "ints": [-2 ** 63, 2 ** 63 - 1, 0, 1, -1],
        "strings": ["", "\x00", "a\x00b", "\x1f\x7f", "\"\\/\b\f\n\r\t",
                    "café", "€", "\U0001f600", "中文" * 20,
                    "x" * 100],
        "metadata": {"name": "n", "labels": {"é": "è", "a/b": "c"},
                     "annotations": {}},
        "status": {"conditions": [{"type": "Ready", "status": "True"}],
                   "nested": [[[]], [{}], [[1.5]]]},
    }
    store = engine.NativeStore(16)
    assert store.put_object("X", "d", "n", tree, None) is True
    assert check_entry(store)
    assert_same_tree(store.fetch_tree(*KEY), tree)
    # sections present in every combination
    for keep in ([], ["metadata"], ["status"], ["kind"], ["metadata", "status"],
                 ["kind", "status"]):
        part = {k: tree[k] for k in tree if k in keep}
        store = engine.NativeStore(16)
        assert store.put_object("X", "d", "n", part, None) is True
        assert check_entry(store)
        assert_same_tree(store.fetch_tree(*KEY), part)


def test_status_splice_keeps_the_member_order_json_loads_gives():
    server = InMemoryApiServer(NativeBackend())
    server.create({"kind": "Pod", "status": {"phase": "Pending"},
                   "metadata": {"name": "n", "namespace": "d"},
                   "spec": {"containers": []}, "apiVersion": "v1"})
    server.mutate_status("Pod", "d", "n",
                         lambda p: p.__setitem__("status", {"phase": "Running"}))
    store = server._backend._store
    assert check_entry(store, ("Pod", "d", "n"))
    assert list(store.fetch_tree("Pod", "d", "n")) == [
        "kind", "spec", "apiVersion", "metadata", "status"]


# -- seeded random trees: zero fallbacks ------------------------------------

ALPHABET = ["a", "b", "key", "app.kubernetes.io/name", "ray.io/cluster", "",
            "é", "x y", "q\"uote", "back\\slash", "\U0001f600", "n\nl",
            "nul\x00", "tab\t", "metadata", "status", "long-" * 12]
LEAF_STRINGS = ALPHABET + ["True", "False", "Running", "10.0.0.1",
                           "rocm/ray:latest", "中文", "\x01\x02",
                           "slash/", "z" * 70]


def random_leaf(rng, odd):
    pick = rng.randrange(8)
    if pick == 0:
        return None
    if pick == 1:
        return rng.random() < 0.5
    if pick == 2:
        return rng.choice([0, 1, -1, 7, 2 ** 31, -2 ** 31, 2 ** 63 - 1, -2 ** 63,
                           rng.randrange(-10 ** 6, 10 ** 6),
                           rng.randrange(-2 ** 63, 2 ** 63)])
    if pick == 3:
        return rng.choice([0.0, -0.0, 0.5, 1e22, 1e-7, 5e-324,
                           1.7976931348623157e308, rng.random(),
                           rng.uniform(-1e6, 1e6), rng.random() * 10 ** rng.randrange(-300, 300),
                           float(rng.randrange(1000))])
    return rng.choice(LEAF_STRINGS)


def random_tree(rng, depth, odd):
    """``odd`` adds what the native encoder declines but json.dumps writes:
    tuples, and int keys (drawn from 1000.., which no str key spells)."""
    if depth <= 0 or rng.random() < 0.3:
        return random_leaf(rng, odd)
    n = rng.randrange(0, 5)
    if rng.random() < 0.55:
        keys = rng.sample(ALPHABET, n)
        out = {k: random_tree(rng, depth - 1, odd) for k in keys}
        if odd and rng.random() < 0.3:
            out[1000 + rng.randrange(50)] = random_tree(rng, depth - 1, odd)
        return out
    items = [random_tree(rng, depth - 1, odd) for _ in range(n)]
    return tuple(items) if odd and rng.random() < 0.3 else items


def has_odd_node(tree):
    if isinstance(tree, tuple):
        return True
    if isinstance(tree, dict):
        return any(not isinstance(k, str) or has_odd_node(v)
                   for k, v in tree.items())
    if isinstance(tree, list):
        return any(has_odd_node(v) for v in tree)
    return False


def test_random_trees_decode_without_fallback():
    rng = random.Random(20240607)
    n_trees, allowed_fallbacks = 300, 0
    fallbacks = sections = blobs = declined = 0
    for i in range(n_trees):
        odd = i % 3 == 2
        tree = random_tree(rng, 4, odd)
        if not isinstance(tree, dict) or i % 2:
            # the server only ever stores objects; other roots go in as blobs
            tree = {"kind": "X", "metadata": {"name": "n", "labels": {}},
                    "spec": tree, "status": random_tree(rng, 2, odd)}
        ways = store_both_ways(tree)
        if len(ways) == 1:
            # tuples and int keys, or a root whose "metadata" is no dict
            declined += 1
            assert has_odd_node(tree) or not isinstance(
                tree.get("metadata", {}), dict)
        for how, store in ways:
            ok = check_entry(store)
            fallbacks += not ok
            sections += how == "sections"
            blobs += how == "blob"
    assert fallbacks <= allowed_fallbacks
    # both paths and the encoder's declines were exercised
    assert blobs == n_trees and sections >= n_trees // 2
    assert declined >= n_trees // 10


# -- no aliasing ---------------------------------------------------------------

def containers(tree, out=None):
    out = {} if out is None else out
    if isinstance(tree, (dict, list)):
        out[id(tree)] = tree
        for v in (tree.values() if isinstance(tree, dict) else tree):
            containers(v, out)
    return out


def assert_disjoint(*trees):
    seen = {}
    for t in trees:
        mine = containers(t)
        assert mine
        assert not (seen.keys() & mine.keys())
        seen.update(mine)


def scramble(tree):
    """Empties every container of ``tree``, innermost last."""
    for c in list(containers(tree).values()):
        c.clear()


def test_results_share_no_containers(bench_server):
    server = bench_server
    backend = server._backend
    assert backend.native_decode
    pod_name = next(p["metadata"]["name"] for p in server.list("Pod")
                    if "worker" in p["metadata"]["name"])
    key = ("Pod", "default", pod_name)
    reference = json.loads(backend._store.fetch(*key))

    a, b = backend.fetch(key), backend.fetch(key)
    assert_same_tree(a, reference)
    assert_disjoint(a, b)
    scramble(a)
    assert_same_tree(b, reference)
    assert_same_tree(backend.fetch(key), reference)

    listed = backend.list("Pod", None, None)
    again = backend.list("Pod", None, None)
    assert len(listed) == 4 and listed == again
    assert_disjoint(b, *listed, *again)
    for tree in listed:
        scramble(tree)
    assert backend.list("Pod", None, None) == again

    first = backend.history_since(0)
    second = backend.history_since(0)
    assert first == second and len(first) > 4
    assert_disjoint(*(obj for _, obj in first), *(obj for _, obj in second))
    for _, obj in first:
        scramble(obj)
    assert backend.history_since(0) == second


def test_deleted_event_object_is_its_own():
    server = InMemoryApiServer(NativeBackend())
    server.create({"kind": "ConfigMap", "metadata": {"name": "c", "namespace": "d",
                                                     "labels": {"a": "b"}},
                   "data": {"k": ["v", {"w": 1}]}})
    fetched = server.get("ConfigMap", "d", "c")
    watcher = server.watch({"ConfigMap"})
    server.delete("ConfigMap", "d", "c")
    (etype, deleted), = watcher.drain()
    assert etype == "DELETED"
    assert deleted["metadata"]["resourceVersion"] == "2"
    replay = server.events_since(0)
    assert [t for t, _ in replay] == ["ADDED", "DELETED"]
    assert replay[1][1] == deleted
    assert_disjoint(fetched, deleted, replay[0][1], replay[1][1])
    expected = json.loads(json.dumps(deleted))
    scramble(deleted)
    scramble(fetched)
    assert server.events_since(0)[1][1] == expected
    # the override of the delete's rv went into the replayed tree only
    assert server.events_since(0)[0][1]["metadata"]["resourceVersion"] == "1"
    assert server._backend.stats()["decode_fallbacks"] == 0


def test_strings_may_be_shared_containers_never():
    store = engine.NativeStore(16)
    store.put_object("X", "d", "n", {"kind": "X", "metadata": {"name": "n"},
                                     "spec": {"phase": "Running"}}, None)
    a, b = store.fetch_tree(*KEY), store.fetch_tree(*KEY)
    assert a == b and a is not b and a["spec"] is not b["spec"]
    # short strings come out of the table: the same object both times
    assert next(iter(a)) is next(iter(b))
    assert a["spec"]["phase"] is b["spec"]["phase"]


def test_intern_table_stays_bounded():
    """Far more distinct short strings than the table has slots: results stay
    right, and the strings it let go of are freed (none is kept twice)."""
    import sys
    store = engine.NativeStore(4)
    for round_ in range(3):
        tree = {"kind": "X",
                "spec": {f"k{round_}-{i}": f"v{round_}-{i}" for i in range(6000)}}
        assert store.put_object("X", "d", "n", tree, None) is not None
        got = store.fetch_tree(*KEY)
        assert_same_tree(got, tree)
    probe = store.fetch_tree(*KEY)["spec"]
    key = next(iter(probe))
    # held by the dict (as key), by `key`, by getrefcount's argument, and at
    # most once by the table
    assert sys.getrefcount(key) <= 4


# -- the switch ----------------------------------------------------------------

def test_switch_off_takes_the_blob_path(monkeypatch):
    backend = NativeBackend()
    monkeypatch.setattr(backend, "native_decode", False)
    backend.put(("X", "d", "n"), {"kind": "X", "metadata": {"name": "n"}})
    assert backend.fetch(("X", "d", "n")) == {"kind": "X",
                                              "metadata": {"name": "n"}}
    assert backend.list("X", None, None) == [{"kind": "X",
                                              "metadata": {"name": "n"}}]
    stats = backend.stats()
    assert stats["trees_decoded"] == 0 and stats["decode_fallbacks"] == 0
    assert stats["blobs_assembled"] == 2
    monkeypatch.setattr(backend, "native_decode", True)
    assert backend.remove(("X", "d", "n")) == {"kind": "X",
                                               "metadata": {"name": "n"}}
    stats = backend.stats()
    assert stats["trees_decoded"] == 1 and stats["blobs_assembled"] == 3


def test_switch_is_read_from_the_environment():
    import subprocess
    import sys
    code = ("from kuberay_amd.kube.native import NativeBackend as B;"
            "print(B.native_decode)")
    root = Path(__file__).resolve().parent.parent
    for value, want in (("0", "False"), ("1", "True"), (None, "True")):
        env = {k: v for k, v in __import__("os").environ.items()
               if k != "KUBERAY_STORE_NATIVE_DECODE"}
        if value is not None:
            env["KUBERAY_STORE_NATIVE_DECODE"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env,
                             capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want
