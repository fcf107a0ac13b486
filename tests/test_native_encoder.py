"""The engine's own JSON encoder and its three-section storage.

The contract on the stored bytes is ``json.loads(blob) == obj`` (not byte
equality with json.dumps); trees the encoder declines must take the
json.dumps path and give exactly what that path always gave."""
import json
import math
import random

import pytest

from kuberay_amd.kube.store import PyBackend

try:
    from kuberay_amd.kube.native import NativeBackend
except ImportError:
    pytest.skip("native engine not built", allow_module_level=True)

try:
    from hypothesis import given, settings, strategies as st
    HAVE_HYPOTHESIS = True
except ImportError:
    HAVE_HYPOTHESIS = False

KEY = ("Thing", "d", "t")


def wrap(value):
    """The value in each of the three sections."""
    return {"kind": "Thing", "spec": {"v": value},
            "metadata": {"name": "t", "namespace": "d", "annotations": {"v": value}},
            "status": {"v": value}}


def nested(depth):
    v = "leaf"
    for i in range(depth):
        v = {"k": v} if i % 2 else [v]
    return v


def roundtrip(obj):
    """(native fetch, python fetch, fallbacks taken)"""
    native, py = NativeBackend(), PyBackend()
    native.put(KEY, obj)
    py.put(KEY, obj)
    return native.fetch(KEY), py.fetch(KEY), native.stats()["fallbacks"]


def same(a, b):
    """Equality that also tells -0.0 from 0.0 and an int from a float."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return (math.isnan(a) and math.isnan(b)) or (
            a == b and math.copysign(1, a) == math.copysign(1, b))
    return a == b


FAST_VALUES = {
    "empty-dict": {},
    "empty-list": [],
    "nested-64": nested(64),
    "control-chars": "".join(chr(c) for c in range(0x20)),
    "each-control-char": [chr(c) for c in range(0x20)],
    "quote-backslash": 'a"b\\c\\"d',
    "u2028": "line\u2028sep\u2029",
    "non-bmp": "ray \U0001F600 \U00010348",
    "latin-cjk": "é ü 漢字",
    "int64-max": 2 ** 63 - 1,
    "int64-min": -2 ** 63,
    "small-ints": [0, -1, 1, 10 ** 18],
    "neg-zero": -0.0,
    "denormal": 1e-320,
    "huge": 1e308,
    "floats": [0.1, 1.5, -2.75e-7, 1e22, 123456789.123456789],
    "scalars": [None, True, False],
    "escaped-key": {'k"\\\n\x01': 1, "": 2},
}


@pytest.mark.parametrize("name", sorted(FAST_VALUES))
def test_fast_path_round_trip(name):
    obj = wrap(FAST_VALUES[name])
    native, py, fallbacks = roundtrip(obj)
    assert same(native, obj)
    assert same(native, py)
    assert fallbacks == 0


class MyStr(str):
    pass


class MyDict(dict):
    pass


FALLBACK_VALUES = {
    "nan": float("nan"),
    "inf": float("inf"),
    "neg-inf": float("-inf"),
    "tuple": (1, "a", [2]),
    "int-key": {1: "a"},
    "none-key": {None: "a"},
    "str-subclass": MyStr("sub"),
    "dict-subclass": MyDict(a=1),
    "lone-surrogate": "\ud800",
    "two-to-63": 2 ** 63,
    "below-int64": -2 ** 63 - 1,
    "two-to-64": 2 ** 64,
    "nested-200": nested(200),
}


@pytest.mark.parametrize("name", sorted(FALLBACK_VALUES))
@pytest.mark.parametrize("where", ["spec", "metadata", "status"])
def test_declined_trees_take_the_json_dumps_path(name, where):
    obj = {"kind": "Thing", "metadata": {"name": "t", "namespace": "d"}}
    if where == "metadata":
        obj["metadata"]["annotations"] = {"v": FALLBACK_VALUES[name]}
    else:
        obj[where] = {"v": FALLBACK_VALUES[name]}
    native = NativeBackend()
    native.put(KEY, obj)
    today = json.loads(json.dumps(obj, separators=(",", ":")))
    assert same(native.fetch(KEY), today)
    assert native.stats()["fallbacks"] == 1
    assert native.stats()["full_encodes"] == 0
    # the blob entry answers everything a native entry does
    assert native.contains(KEY) and native.count("Thing") == 1
    assert native.peek(KEY) == ("", "", False, "")
    # a status write on a blob entry cannot splice: full write instead
    got = native.fetch(KEY)
    got["status"] = {"phase": "x"}
    native.put_status(KEY, got)
    assert native.fetch(KEY)["status"] == {"phase": "x"}
    assert native.kinds() == ["Thing"]
    assert same(native.remove(KEY), native_expected(today, got))


def native_expected(today, got):
    out = dict(today)
    out["status"] = got["status"]
    return out


def test_top_level_that_is_no_plain_dict_falls_back():
    native = NativeBackend()
    native.put(KEY, MyDict(kind="Thing", metadata={"name": "t"}))
    assert native.fetch(KEY) == {"kind": "Thing", "metadata": {"name": "t"}}
    assert native.stats()["fallbacks"] == 1


def test_circular_structure_raises_what_json_dumps_raises():
    loop = {"kind": "Thing", "metadata": {"name": "t"}, "spec": {}}
    loop["spec"]["self"] = loop
    with pytest.raises(ValueError) as today:
        json.dumps(loop, separators=(",", ":"))
    native = NativeBackend()
    with pytest.raises(ValueError) as got:
        native.put(KEY, loop)
    assert str(got.value) == str(today.value)
    assert not native.contains(KEY)
    assert native.kinds() == []
    # and no Python error is left behind by the declined fast path
    native.put(KEY, wrap(1))
    assert native.fetch(KEY) == wrap(1)


def test_fields_the_old_path_rejects_are_still_rejected():
    """resourceVersion None was a TypeError at the binding; it still is."""
    native = NativeBackend()
    with pytest.raises(TypeError):
        native.put(KEY, {"kind": "Thing",
                         "metadata": {"name": "t", "resourceVersion": None}})
    assert not native.contains(KEY)


# -- randomized sweep -------------------------------------------------------

def _random_value(rng, depth=0):
    kinds = ["str", "int", "float", "bool", "none"]
    if depth < 4:
        kinds += ["dict", "list"] * 2
    kind = rng.choice(kinds)
    if kind == "str":
        alphabet = ['a', 'Z', '"', '\\', '\n', '\x00', '\x1f', ' ', '/', 'é',
                    '\u2028', '\x7f', '\U0001F600', '漢']
        return "".join(rng.choice(alphabet) for _ in range(rng.randrange(6)))
    if kind == "int":
        return rng.choice([0, 1, -1, 2 ** 31, 2 ** 63 - 1, -2 ** 63, 2 ** 63,
                           2 ** 64, rng.randrange(-10 ** 6, 10 ** 6)])
    if kind == "float":
        return rng.choice([0.0, -0.0, 1e-320, 1e308, rng.uniform(-1e6, 1e6),
                           rng.random()])
    if kind == "bool":
        return rng.random() < 0.5
    if kind == "none":
        return None
    if kind == "list":
        return [_random_value(rng, depth + 1) for _ in range(rng.randrange(4))]
    return {_random_value_key(rng): _random_value(rng, depth + 1)
            for _ in range(rng.randrange(4))}


def _random_value_key(rng):
    return "".join(rng.choice('ab"\\\né\x07') for _ in range(rng.randrange(1, 4)))


def _check_sweep_value(value):
    obj = wrap(value)
    native, py, _ = roundtrip(obj)
    assert same(native, obj)
    assert same(native, py)


if HAVE_HYPOTHESIS:
    _json_values = st.recursive(
        st.none() | st.booleans() | st.integers()
        | st.floats(allow_nan=False, allow_infinity=False) | st.text(),
        lambda children: st.lists(children, max_size=4)
        | st.dictionaries(st.text(max_size=6), children, max_size=4),
        max_leaves=20)

    @settings(max_examples=150, deadline=None)
    @given(_json_values)
    def test_round_trip_sweep(value):
        _check_sweep_value(value)
else:
    def test_round_trip_sweep():
        rng = random.Random(20240607)
        for _ in range(300):
            _check_sweep_value(_random_value(rng))


def test_round_trip_sweep_seeded():
    """The same sweep from a fixed seed (runs with or without hypothesis;
    its alphabet is all escapes and boundaries)."""
    rng = random.Random(7)
    for _ in range(200):
        _check_sweep_value(_random_value(rng))


# -- pod view: the native extraction against compute_pod_view ---------------

def _random_pod(rng, i):
    def maybe(*choices):
        return rng.choice(choices)
    status = maybe(None, {}, "absent", {
        "phase": maybe("Running", "Pending", "", None),
        "podIP": maybe("10.0.0.1", None, ""),
        "conditions": maybe(None, [], [
            {"type": "Ready", "status": maybe("True", "False")},
            {"type": maybe("Ready", "Initialized"), "status": "True"}]),
        "containerStatuses": maybe(None, [], [
            {"name": maybe("ray", "side", None),
             "state": maybe(None, {}, {"terminated": maybe({}, {"exitCode": 1}, None)},
                            {"running": {}})},
            {"state": {"terminated": {"exitCode": 2}}}]),
    })
    spec = maybe(None, {}, "absent", {
        "restartPolicy": maybe("Never", "Always", None, ""),
        "containers": maybe(None, [], [{"name": maybe("ray", None)}, {"name": "side"}],
                            [{}]),
    })
    meta = {"name": f"p{i}", "namespace": maybe("d", "e"),
            "labels": maybe(None, {}, {"g": maybe("x", "y"), "h": "z"}),
            "resourceVersion": str(i)}
    if rng.random() < 0.5:
        meta["creationTimestamp"] = "2024-01-01T00:00:00Z"
    if rng.random() < 0.3:
        meta["deletionTimestamp"] = maybe("2024-01-02T00:00:00Z", None, "")
    pod = {"kind": "Pod", "metadata": meta}
    if spec != "absent":
        pod["spec"] = spec
    if status != "absent":
        pod["status"] = status
    return pod


def test_pod_view_matches_compute_pod_view():
    rng = random.Random(11)
    native, py = NativeBackend(), PyBackend()
    for i in range(300):
        pod = _random_pod(rng, i)
        key = ("Pod", pod["metadata"]["namespace"], pod["metadata"]["name"])
        native.put(key, pod)
        py.put(key, pod)
    assert native.stats()["fallbacks"] == 0
    assert native.list_views(None, None) == py.list_views(None, None)
    assert native.list_views("d", {"g": "x"}) == py.list_views("d", {"g": "x"})
    # and again after status-only writes
    for i in range(300):
        pod = _random_pod(rng, i)
        key = ("Pod", pod["metadata"]["namespace"], pod["metadata"]["name"])
        stored = py.fetch(key)
        if stored is None:
            continue
        if "status" in pod:
            stored["status"] = pod["status"]
        native.put_status(key, stored)
        py.put(key, stored)
    assert native.stats()["partial_encodes"] > 0
    assert native.list_views(None, None) == py.list_views(None, None)
    assert native.list("Pod", None, None) == py.list("Pod", None, None)


# -- sections ---------------------------------------------------------------

SECTION_OBJECTS = {
    "no-status": {"kind": "ConfigMap", "metadata": {"name": "t", "namespace": "d"},
                  "data": {"a": "b"}},
    "secret-no-spec": {"apiVersion": "v1", "kind": "Secret", "type": "Opaque",
                       "metadata": {"name": "t", "namespace": "d",
                                    "labels": {"g": "x"}},
                       "data": {"password": "aHVudGVyMg=="}},
    "status-none": {"kind": "Thing", "metadata": {"name": "t"}, "spec": {"a": 1},
                    "status": None},
    "status-string": {"kind": "Thing", "metadata": {"name": "t"}, "status": "ok"},
    "status-number": {"kind": "Thing", "metadata": {"name": "t"}, "status": 7},
    "status-list": {"kind": "Thing", "metadata": {"name": "t"}, "status": [1, {"a": 2}]},
    "status-first": {"status": {"phase": "P"}, "spec": {"a": [1, 2]},
                     "kind": "Thing", "apiVersion": "v9",
                     "metadata": {"name": "t", "namespace": "d"}},
    "metadata-only": {"metadata": {"name": "t"}},
    "no-metadata": {"kind": "Thing", "spec": {"a": 1}},
    "status-only": {"status": {"a": 1}},
    "empty": {},
}


@pytest.mark.parametrize("name", sorted(SECTION_OBJECTS))
def test_sections_assemble_to_the_object(name):
    obj = SECTION_OBJECTS[name]
    native, py, fallbacks = roundtrip(obj)
    assert same(native, obj)
    assert same(native, py)
    assert fallbacks == 0
    backend = NativeBackend()
    backend.put(KEY, obj)
    assert backend.list("Thing", None, None) == [obj]
    compact = json.dumps(obj, separators=(",", ":"))
    # one allocation's worth: the sections are the compact encoding plus the
    # two member names, counted once
    assert backend.total_bytes() <= len(compact)
    assert backend.total_bytes() >= len(compact) - len('{,"metadata":,"status":}')


@pytest.mark.parametrize("name", sorted(SECTION_OBJECTS))
def test_status_write_encodes_metadata_and_status_only(name):
    obj = json.loads(json.dumps(SECTION_OBJECTS[name]))
    obj.setdefault("metadata", {})["resourceVersion"] = "1"
    obj["spec"] = {"big": ["x" * 50] * 40, "containers": [{"name": "ray"}]}
    backend = NativeBackend()
    backend.put(KEY, obj)
    before = backend.stats()
    new = backend.fetch(KEY)
    new["status"] = {"phase": "Running", "n": [1, 2, 3]}
    new["metadata"]["resourceVersion"] = "2"
    backend.put_status(KEY, new)
    after = backend.stats()
    budget = (len(json.dumps(new["metadata"], separators=(",", ":")))
              + len(json.dumps(new["status"], separators=(",", ":"))) + 16)
    assert after["bytes_encoded"] - before["bytes_encoded"] <= budget
    assert after["partial_encodes"] == before["partial_encodes"] + 1
    assert after["full_encodes"] == before["full_encodes"]
    got = backend.fetch(KEY)
    assert got == new
    for k in obj:
        if k not in ("metadata", "status"):
            assert got[k] == obj[k]
    assert backend.rv(KEY) == "2"
    assert backend.peek(KEY)[0] == "2"


def test_top_level_order_of_the_rest_is_kept():
    obj = SECTION_OBJECTS["status-first"]
    backend = NativeBackend()
    backend.put(KEY, obj)
    keys = [k for k in backend.fetch(KEY) if k not in ("metadata", "status")]
    assert keys == ["spec", "kind", "apiVersion"]
