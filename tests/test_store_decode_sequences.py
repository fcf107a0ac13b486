"""One seeded operation sequence on three servers: NativeBackend reading
through the section decoder, NativeBackend with it switched off
(KUBERAY_STORE_NATIVE_DECODE=0: blob + json.loads) and PyBackend. Every
returned object, every watch event, every history replay and the final state
must be equal. Some of the objects carry what the decoder hands back to
json.loads (an integer past int64), so the per-object fallback runs inside
lists and history replays too."""
import itertools
import random
import types

import pytest

from kuberay_amd.kube import store as store_mod
from kuberay_amd.kube.store import (AlreadyExistsError, ApiError,
                                    ConflictError, InMemoryApiServer,
                                    NotFoundError, PyBackend)

try:
    from kuberay_amd.kube.native import NativeBackend
except ImportError:
    pytest.skip("native engine not built", allow_module_level=True)


@pytest.fixture
def ids(monkeypatch):
    """uids and timestamps as a pure function of call order."""
    state = types.SimpleNamespace(counter=itertools.count())

    class Uid:
        def __init__(self, n):
            self.hex = f"{n:05x}" + "0" * 27

        def __str__(self):
            return f"uid-{self.hex}"

    monkeypatch.setattr(store_mod, "uuid", types.SimpleNamespace(
        uuid4=lambda: Uid(next(state.counter))))
    monkeypatch.setattr(store_mod, "now_iso", lambda: "2024-06-07T00:00:00Z")
    state.reset = lambda: setattr(state, "counter", itertools.count())
    return state


NAMES = ["a", "b", "c"]
KINDS = ["ConfigMap", "Pod", "Service"]


def new_object(kind, name, n):
    meta = {"name": name, "namespace": "d",
            "labels": {"g": "x", "app.kubernetes.io/name": f"n{n % 3}"},
            "annotations": {"note": "café \U0001f600 \"q\" \\ \n" * (n % 3)}}
    if n % 5 == 0:
        meta["finalizers"] = ["f"]
    if kind == "Pod":
        obj = {"apiVersion": "v1", "kind": "Pod", "metadata": meta,
               "spec": {"containers": [{"name": "ray", "image": "rocm/ray:latest",
                                        "env": [{"name": "N", "value": str(n)}]}],
                        "restartPolicy": "Never"},
               "status": {"phase": "Pending"}}
    elif kind == "Service":
        obj = {"kind": "Service", "metadata": meta,
               "spec": {"clusterIP": f"10.0.0.{n}",
                        "ports": [{"name": "p", "port": 8000 + n}]}}
    else:
        obj = {"kind": kind, "metadata": meta,
               "data": {"k": [n, n / 7, -0.0, None, True, {"deep": [[], {}]}]}}
    if n % 7 == 0:
        obj["spec"] = dict(obj.get("spec") or {}, big=2 ** 70 + n)
    return obj


def apply_op(server, rng):
    """One random operation; returns a comparable observation. The random
    choices are drawn before the server is touched."""
    op = rng.choice(["create", "create", "create", "get", "list", "list_sel",
                     "update_spec", "update_status", "mutate", "patch",
                     "patch_status", "clear_finalizers", "delete", "delete",
                     "stale_update", "replay"])
    kind, name, n = rng.choice(KINDS), rng.choice(NAMES), rng.randrange(100)
    try:
        if op == "create":
            return ("created", server.create(new_object(kind, name, n)))
        if op == "get":
            return ("got", server.get(kind, "d", name),
                    server.try_get(kind, "d", name))
        if op == "list":
            return ("listed", server.list(kind))
        if op == "list_sel":
            return ("selected", server.list(
                kind, "d", {"app.kubernetes.io/name": f"n{n % 3}"}))
        if op == "update_spec":
            cur = server.get(kind, "d", name)
            cur["spec"] = dict(cur.get("spec") or {}, v=n, f=n / 3)
            return ("updated", server.update(cur))
        if op == "update_status":
            cur = server.get(kind, "d", name)
            cur["status"] = {"phase": "S", "n": n, "ratio": 1e22 * n}
            return ("status", server.update(cur, subresource="status"))
        if op == "stale_update":
            cur = server.get(kind, "d", name)
            cur["metadata"]["resourceVersion"] = "0"
            return ("stale", server.update(cur))
        if op == "mutate":
            def fn(obj):
                obj.setdefault("status", {})["n"] = n
            return ("mutated", server.mutate_status(kind, "d", name, fn))
        if op == "patch":
            return ("patched", server.patch_merge(
                kind, "d", name,
                {"spec": {"v": n, "gone": None, "nested": {"k": [n]}},
                 "metadata": {"labels": {"g": "y" if n % 2 else None}}}))
        if op == "patch_status":
            return ("patched-status", server.patch_merge(
                kind, "d", name, {"status": {"phase": "Running", "n": n}},
                subresource="status"))
        if op == "clear_finalizers":
            cur = server.get(kind, "d", name)
            cur["metadata"]["finalizers"] = []
            return ("unfinalized", server.update(cur))
        if op == "delete":
            server.delete(kind, "d", name)
            return ("deleted",)
        if op == "replay":
            since = max(server.current_rv - n % 10, 0)
            return ("replayed", server.events_since(since),
                    server.events_since(since, {kind}))
    except NotFoundError:
        return ("not_found",)
    except AlreadyExistsError:
        return ("exists",)
    except ConflictError:
        return ("conflict",)
    except ApiError as e:
        return ("api_error", e.code)
    raise AssertionError(op)


def observe(server):
    return {
        "objects": {k: server.list(k) for k in KINDS},
        "views": server.list_pod_views(),
        "service_views": [server.service_view("d", n) for n in NAMES],
        "counts": {k: server.count(k) for k in KINDS},
        "rv": server.current_rv,
        "history": [server.events_since(rv)
                    for rv in range(0, server.current_rv + 1, 7)],
    }


def run_sequence(server, seed, n_ops):
    rng = random.Random(seed)
    watcher = server.watch()
    results = [apply_op(server, rng) for _ in range(n_ops)]
    return results, watcher.drain()


def test_sequence_matches_with_the_decoder_on_off_and_on_pybackend(ids,
                                                                   monkeypatch):
    runs = {}
    for label, make, decode in (("py", PyBackend, None),
                                ("native-on", NativeBackend, True),
                                ("native-off", NativeBackend, False)):
        ids.reset()
        backend = make()
        if decode is not None:
            monkeypatch.setattr(backend, "native_decode", decode, raising=True)
        server = InMemoryApiServer(backend=backend)
        results, events = run_sequence(server, seed=7, n_ops=400)
        runs[label] = (server, results, events)

    py, py_results, py_events = runs["py"]
    assert py.current_rv < InMemoryApiServer.EVENT_HISTORY_LIMIT
    for label in ("native-on", "native-off"):
        server, results, events = runs[label]
        for i, (a, b) in enumerate(zip(py_results, results)):
            assert a == b, (label, i, a[0])
        assert events == py_events, label
        assert observe(server) == observe(py), label

    # the sequence did what it is meant to
    kinds_of_result = {r[0] for r in py_results}
    assert {"created", "got", "listed", "selected", "updated", "status",
            "mutated", "patched", "patched-status", "unfinalized", "deleted",
            "replayed", "not_found", "exists", "conflict"} <= kinds_of_result
    assert {t for t, _ in py_events} == {"ADDED", "MODIFIED", "DELETED"}

    on = runs["native-on"][0]._backend.stats()
    off = runs["native-off"][0]._backend.stats()
    assert off["trees_decoded"] == 0 and off["decode_fallbacks"] == 0
    assert on["trees_decoded"] > 0
    # the big-int objects: written as blobs, handed back as blobs
    assert on["fallbacks"] > 0 and on["decode_fallbacks"] > 0
    # a reader got the same number of objects either way
    assert on["trees_decoded"] + on["decode_fallbacks"] == on["blobs_assembled"]
    assert on["blobs_assembled"] == off["blobs_assembled"]
    assert on["bytes_assembled"] == off["bytes_assembled"]
