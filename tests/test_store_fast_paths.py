"""InMemoryApiServer over the engine's fast paths (one native call per write,
status splice, peek-decided delete, history ring in the engine) against the
same server over PyBackend, which keeps the plain put/fetch/remove protocol
and the python history."""
import itertools
import json
import random
import threading
import types

import pytest

from kuberay_amd.kube import store as store_mod
from kuberay_amd.kube.snapshot import load_snapshot, save_snapshot
from kuberay_amd.kube.store import (AlreadyExistsError, ApiError,
                                    ConflictError, InMemoryApiServer,
                                    NotFoundError, PyBackend)

try:
    from kuberay_amd.kube import native as native_mod
    from kuberay_amd.kube.native import NativeBackend
except ImportError:
    pytest.skip("native engine not built", allow_module_level=True)


@pytest.fixture
def ids(monkeypatch):
    """uids and timestamps as a pure function of call order, so two servers
    fed the same operations must agree byte for byte. ``ids.reset()``
    restarts the sequence before the second server's run."""
    state = types.SimpleNamespace(counter=itertools.count())

    class Uid:
        def __init__(self, n):
            self.hex = f"{n:032x}"

        def __str__(self):
            return f"uid-{self.hex}"

    monkeypatch.setattr(store_mod, "uuid", types.SimpleNamespace(
        uuid4=lambda: Uid(next(state.counter))))
    monkeypatch.setattr(store_mod, "now_iso", lambda: "2024-06-07T00:00:00Z")
    state.reset = lambda: setattr(state, "counter", itertools.count())
    return state


POD_SPEC = {"containers": [{"name": "ray", "image": "rocm/ray:latest",
                            "resources": {"limits": {"amd.com/gpu": "1"}}}],
            "restartPolicy": "Never"}


def pod(name, **meta):
    return {"apiVersion": "v1", "kind": "Pod",
            "metadata": dict({"name": name, "namespace": "d",
                              "labels": {"g": "x"}}, **meta),
            "spec": json.loads(json.dumps(POD_SPEC)),
            "status": {"phase": "Pending"}}


# -- 3. work counters over one pod lifecycle ---------------------------------

def test_pod_lifecycle_encodes_once_and_never_calls_json_dumps(monkeypatch):
    the_pod = pod("p")  # built before json.dumps is counted
    calls = []
    real = json.dumps

    def counting(*args, **kwargs):
        calls.append(args)
        return real(*args, **kwargs)

    monkeypatch.setattr(json, "dumps", counting)
    monkeypatch.setattr(native_mod, "_dumps", counting)
    server = InMemoryApiServer(backend=NativeBackend())
    watcher = server.watch({"Pod"})

    server.create(the_pod)

    def to_running(obj):
        obj["status"] = {"phase": "Running", "podIP": "10.0.0.1",
                         "conditions": [{"type": "Ready", "status": "True"}]}

    out = server.mutate_status("Pod", "d", "p", to_running)
    assert out["status"]["phase"] == "Running"
    assert server.list_pod_views("d")[0].ready
    server.delete("Pod", "d", "p")

    stats = server._backend.stats()
    assert stats["full_encodes"] == 1
    assert stats["partial_encodes"] == 1
    assert stats["blobs_assembled"] == 2
    assert stats["fallbacks"] == 0
    assert stats["history_appends"] == 3
    assert calls == []
    events = watcher.drain()
    assert [e[0] for e in events] == ["ADDED", "MODIFIED", "DELETED"]
    assert [int(e[1]["metadata"]["resourceVersion"]) for e in events] == [1, 2, 3]
    assert server.count("Pod") == 0


# -- 4 + 5. one seeded operation sequence on both servers -------------------

NAMES = ["a", "b", "c", "d"]
KINDS = ["ConfigMap", "Pod", "RayCluster"]


def apply_op(server, rng):
    """One random operation; returns a comparable observation. The random
    choices are drawn before the server is touched, so both servers see the
    same sequence."""
    op = rng.choice(["create", "create", "chain", "update_spec", "update_status",
                     "mutate", "mutate_skip", "patch", "patch_status",
                     "add_finalizer", "clear_finalizers", "delete", "delete",
                     "stale_update"])
    kind, name, n = rng.choice(KINDS), rng.choice(NAMES), rng.randrange(100)
    try:
        if op == "create":
            obj = pod(name) if kind == "Pod" else {
                "kind": kind, "metadata": {"name": name, "namespace": "d"},
                "spec": {"v": n}}
            if n % 5 == 0:
                obj["metadata"]["finalizers"] = ["f"]
            return ("created", server.create(obj))
        if op == "chain":
            # owner -> child -> grandchild, one dependent each: the order a
            # cascade visits several dependents of one owner in is
            # unspecified (set order) in either backend
            out = []
            owner = server.try_get("RayCluster", "d", "own") or server.create(
                {"kind": "RayCluster", "metadata": {"name": "own", "namespace": "d"}})
            child = server.try_get("Pod", "d", "child") or server.create(
                pod("child", ownerReferences=[
                    {"kind": "RayCluster", "name": "own",
                     "uid": owner["metadata"]["uid"]}]))
            out.append(child)
            if n % 2:
                out.append(server.try_get("ConfigMap", "d", "grand") or server.create(
                    {"kind": "ConfigMap",
                     "metadata": {"name": "grand", "namespace": "d",
                                  "finalizers": ["f"] if n % 3 == 0 else [],
                                  "ownerReferences": [
                                      {"kind": "Pod", "name": "child",
                                       "uid": child["metadata"]["uid"]}]}}))
            return ("chain", out)
        if op == "delete" and n % 4 == 0:
            server.delete("RayCluster", "d", "own")
            return ("deleted-owner",)
        if op == "update_spec":
            cur = server.get(kind, "d", name)
            cur["spec"] = dict(cur.get("spec") or {}, v=n)
            return ("updated", server.update(cur))
        if op == "update_status":
            cur = server.get(kind, "d", name)
            cur["status"] = {"phase": "S", "n": n}
            cur["spec"] = {"ignored": True}
            return ("status", server.update(cur, subresource="status"))
        if op == "stale_update":
            cur = server.get(kind, "d", name)
            cur["metadata"]["resourceVersion"] = "0"
            return ("stale", server.update(cur))
        if op == "mutate":
            def fn(obj):
                obj.setdefault("status", {})["n"] = n
            return ("mutated", server.mutate_status(kind, "d", name, fn))
        if op == "mutate_skip":
            return ("skipped", server.mutate_status(kind, "d", name,
                                                    lambda obj: False))
        if op == "patch":
            return ("patched", server.patch_merge(
                kind, "d", name,
                {"spec": {"v": n, "gone": None, "nested": {"k": [n]}},
                 "metadata": {"labels": {"g": "y" if n % 2 else None}}}))
        if op == "patch_status":
            patch = {"status": {"phase": "Running", "n": n}} if n % 2 else {"n": n}
            return ("patched-status", server.patch_merge(
                kind, "d", name, patch, subresource="status"))
        if op == "add_finalizer":
            cur = server.get(kind, "d", name)
            cur["metadata"]["finalizers"] = ["f"]
            return ("finalized", server.update(cur))
        if op == "clear_finalizers":
            cur = server.get(kind, "d", name)
            cur["metadata"]["finalizers"] = []
            return ("unfinalized", server.update(cur))
        if op == "delete":
            server.delete(kind, "d", name)
            return ("deleted",)
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
        "selected": server.list("Pod", "d", {"g": "x"}),
        "counts": {k: server.count(k) for k in KINDS},
        "kinds": sorted(server.kinds()),
        "rv": server.current_rv,
    }


def run_sequence(server, seed, n_ops):
    rng = random.Random(seed)
    watcher = server.watch()
    results = [apply_op(server, rng) for _ in range(n_ops)]
    return results, watcher.drain()


@pytest.fixture
def both_after_sequence(ids):
    out = []
    for backend in (PyBackend(), NativeBackend()):
        ids.reset()
        server = InMemoryApiServer(backend=backend)
        results, events = run_sequence(server, seed=42, n_ops=500)
        out.append((server, results, events))
    return out


def test_sequence_results_events_and_state_match(both_after_sequence):
    (py, py_results, py_events), (native, nat_results, nat_events) = both_after_sequence
    for i, (a, b) in enumerate(zip(py_results, nat_results)):
        assert a == b, (i, a, b)
    assert py_events == nat_events
    assert observe(py) == observe(native)
    assert native._backend.stats()["fallbacks"] == 0
    # the sequence exercised what it is meant to
    kinds_of_result = {r[0] for r in py_results}
    assert {"created", "chain", "deleted-owner", "updated", "status", "mutated",
            "skipped", "patched", "patched-status", "finalized", "unfinalized",
            "deleted", "not_found", "exists", "conflict"} <= kinds_of_result
    assert any(e[0] == "DELETED" for e in py_events)


def test_history_matches_for_every_rv(both_after_sequence):
    (py, _, py_events), (native, _, _) = both_after_sequence
    assert py.current_rv == native.current_rv
    assert py.current_rv < InMemoryApiServer.EVENT_HISTORY_LIMIT
    for rv in range(py.current_rv + 2):
        a, b = py.events_since(rv), native.events_since(rv)
        assert a == b, rv
        assert a is not None
    everything = native.events_since(0)
    assert everything == py_events
    # a DELETED event carries the delete's own, fresh rv
    rvs = [int(obj["metadata"]["resourceVersion"]) for _, obj in everything]
    assert rvs == sorted(set(rvs))
    assert any(t == "DELETED" for t, _ in everything)
    for kinds in ({"Pod"}, {"ConfigMap", "RayCluster"}, set()):
        assert py.events_since(3, kinds) == native.events_since(3, kinds)


def test_history_eviction_matches(ids):
    limit = InMemoryApiServer.EVENT_HISTORY_LIMIT
    servers = []
    for backend in (PyBackend(), NativeBackend()):
        ids.reset()
        server = InMemoryApiServer(backend=backend)
        rng = random.Random(5)
        while server.current_rv < limit + 150:
            name = f"c{rng.randrange(40)}"
            try:
                if rng.random() < 0.3:
                    server.delete("ConfigMap", "d", name)
                else:
                    server.create({"kind": "ConfigMap",
                                   "metadata": {"name": name, "namespace": "d"}})
            except (NotFoundError, AlreadyExistsError):
                pass
        servers.append(server)
    py, native = servers
    assert py.current_rv == native.current_rv > limit
    oldest = py.current_rv - limit + 1  # rv of the oldest retained event
    # every rv in the evicted range and around its edge; inside the retained
    # window (where test_history_matches_for_every_rv already walks every
    # rv) a stride, since each replay there decodes up to 1024 objects
    rvs = (set(range(oldest + 3)) | set(range(oldest, py.current_rv, 97))
           | set(range(py.current_rv - 2, py.current_rv + 2)))
    gone = 0
    for rv in sorted(rvs):
        a = py.events_since(rv)
        assert native.events_since(rv) == a, rv
        if a is None:
            assert rv + 1 < oldest
            gone += 1
    assert gone == oldest - 1
    assert len(native.events_since(oldest - 1)) == limit


def test_history_after_snapshot_restore_matches(both_after_sequence, tmp_path, ids):
    (py, _, _), (native, _, _) = both_after_sequence
    restored = []
    for source, backend in ((py, PyBackend()), (native, NativeBackend())):
        path = str(tmp_path / f"{source.backend_name}.jsonl")
        assert save_snapshot(source, path) > 0
        server = InMemoryApiServer(backend=backend)
        assert load_snapshot(server, path) > 0
        restored.append(server)
    new_py, new_native = restored
    base = py.current_rv
    assert new_py.current_rv == new_native.current_rv == base
    assert observe(new_py) == observe(new_native) == observe(py)
    for rv in (0, 1, base - 1):
        assert new_py.events_since(rv) is None
        assert new_native.events_since(rv) is None
    assert new_py.events_since(base) == new_native.events_since(base) == []
    for server in restored:
        ids.reset()
        run_sequence(server, seed=43, n_ops=60)
    assert new_py.current_rv == new_native.current_rv > base
    for rv in range(base - 1, new_py.current_rv + 2):
        assert new_py.events_since(rv) == new_native.events_since(rv), rv


def test_history_is_in_strict_rv_order_under_concurrent_writers():
    server = InMemoryApiServer(backend=NativeBackend())
    errors = []

    def writer(t):
        try:
            for i in range(100):
                name = f"w{t}-{i % 7}"
                try:
                    server.create({"kind": "ConfigMap",
                                   "metadata": {"name": name, "namespace": "d"}})
                except AlreadyExistsError:
                    server.patch_merge("ConfigMap", "d", name, {"data": {"i": str(i)}})
                if i % 5 == 4:
                    server.delete("ConfigMap", "d", name)
        except Exception as e:  # pragma: no cover
            errors.append(e)

    threads = [threading.Thread(target=writer, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    rvs = server._backend.history_rvs()
    assert len(rvs) == min(server.current_rv, server.EVENT_HISTORY_LIMIT)
    assert all(a < b for a, b in zip(rvs, rvs[1:]))
    assert rvs[-1] == server.current_rv
    replay = server.events_since(rvs[0])
    assert [int(o["metadata"]["resourceVersion"]) for _, o in replay] == rvs[1:]


# -- 5. named semantics, backend against backend ------------------------------

def scenario_results(ids, scenario):
    out = []
    for backend in (PyBackend(), NativeBackend()):
        ids.reset()
        server = InMemoryApiServer(backend=backend)
        watcher = server.watch()
        result = scenario(server)
        out.append((result, watcher.drain(), observe(server),
                    server.events_since(0)))
    assert out[0] == out[1]
    return out[1]


def test_mutate_status_semantics(ids):
    def scenario(server):
        created = server.create(pod("p", finalizers=["f"]))
        seen = []

        def fn(obj):
            seen.append(json.loads(json.dumps(obj)))
            obj["status"]["phase"] = "Running"
            obj["status"]["podIP"] = "10.1.1.1"
        first = server.mutate_status("Pod", "d", "p", fn)
        skipped = server.mutate_status("Pod", "d", "p", lambda o: False)
        missing = server.mutate_status("Pod", "d", "nope", fn)
        return created, first, skipped, missing, seen, server.get("Pod", "d", "p")

    (created, first, skipped, missing, seen, stored), events, _, _ = \
        scenario_results(ids, scenario)
    assert skipped is None and missing is None
    assert seen == [created]
    assert first == stored
    assert first["metadata"]["resourceVersion"] == "2"
    assert first["metadata"]["generation"] == 1
    assert first["metadata"]["uid"] == created["metadata"]["uid"]
    assert first["spec"] == created["spec"]
    assert [e[0] for e in events] == ["ADDED", "MODIFIED"]


def test_patch_merge_semantics_both_subresources(ids):
    def scenario(server):
        server.create(pod("p"))
        a = server.patch_merge("Pod", "d", "p", {
            "spec": {"restartPolicy": "Always"},
            "metadata": {"labels": {"h": "z", "g": None}},
            "status": {"phase": "ignored-by-main-resource"}})
        b = server.patch_merge("Pod", "d", "p", {"status": {"phase": "Running"}},
                               subresource="status")
        c = server.patch_merge("Pod", "d", "p", {"podIP": "10.0.0.2"},
                               subresource="status")
        d = server.patch_merge("Pod", "d", "p", {"metadata": {"annotations": {"a": "1"}}})
        with pytest.raises(ConflictError):
            server.patch_merge("Pod", "d", "p",
                               {"metadata": {"resourceVersion": "1"}})
        with pytest.raises(NotFoundError):
            server.patch_merge("Pod", "d", "nope", {"spec": {}})
        return a, b, c, d, server.list("Pod", "d", {"h": "z"}), \
            server.list("Pod", "d", {"g": "x"})

    (a, b, c, d, by_h, by_g), _, state, _ = scenario_results(ids, scenario)
    assert a["metadata"]["generation"] == 2          # spec changed
    assert a["status"] == {"phase": "Pending"}       # status is not patchable here
    assert a["metadata"]["labels"] == {"h": "z"}
    assert b["status"] == {"phase": "Running"} and b["metadata"]["generation"] == 2
    assert c["status"] == {"phase": "Running", "podIP": "10.0.0.2"}
    assert d["metadata"]["generation"] == 2          # spec unchanged
    assert [o["metadata"]["name"] for o in by_h] == ["p"] and by_g == []
    assert state["views"][0].phase == "Running"
    assert state["views"][0].pod_ip == "10.0.0.2"
    assert state["views"][0].restart_policy == "Always"


def test_finalizer_blocked_delete_then_removal_deletes(ids):
    def scenario(server):
        server.create(pod("p", finalizers=["f"]))
        server.delete("Pod", "d", "p")
        blocked = server.get("Pod", "d", "p")
        rv_after_first = server.current_rv
        server.delete("Pod", "d", "p")               # already terminating
        assert server.current_rv == rv_after_first
        status = server.mutate_status(
            "Pod", "d", "p", lambda o: o["status"].update(phase="Failed"))
        cur = server.get("Pod", "d", "p")
        cur["metadata"]["finalizers"] = []
        server.update(cur)
        with pytest.raises(NotFoundError):
            server.delete("Pod", "d", "p")
        return blocked, status, server.try_get("Pod", "d", "p")

    (blocked, status, after), events, state, history = scenario_results(ids, scenario)
    assert blocked["metadata"]["deletionTimestamp"]
    assert blocked["metadata"]["resourceVersion"] == "2"
    assert status["metadata"]["deletionTimestamp"]   # carried over
    assert after is None and state["counts"]["Pod"] == 0
    assert [e[0] for e in events] == ["ADDED", "MODIFIED", "MODIFIED",
                                      "MODIFIED", "DELETED"]
    assert [int(o["metadata"]["resourceVersion"]) for _, o in history] == [1, 2, 3, 4, 5]


def test_owner_garbage_collection(ids):
    def scenario(server):
        owner = server.create({"kind": "RayCluster",
                               "metadata": {"name": "c", "namespace": "d"}})
        ref = [{"kind": "RayCluster", "name": "c", "uid": owner["metadata"]["uid"]}]
        child = server.create(pod("child", ownerReferences=ref))
        server.create({"kind": "ConfigMap", "metadata": {
            "name": "grand", "namespace": "d", "finalizers": ["keep"],
            "ownerReferences": [{"kind": "Pod", "name": "child",
                                 "uid": child["metadata"]["uid"]}]}})
        server.create(pod("bystander"))
        server.delete("RayCluster", "d", "c")
        return (server.try_get("Pod", "d", "child"),
                server.get("ConfigMap", "d", "grand"),
                server._backend.dependents(owner["metadata"]["uid"]))

    (child, grand, deps), events, state, _ = scenario_results(ids, scenario)
    assert child is None
    assert grand["metadata"]["deletionTimestamp"]    # blocked by its finalizer
    assert deps == []
    assert state["counts"] == {"ConfigMap": 1, "Pod": 1, "RayCluster": 0}
    assert [e[0] for e in events][-3:] == ["DELETED", "DELETED", "MODIFIED"]


# -- 6. concurrency -----------------------------------------------------------

@pytest.mark.parametrize("backend_cls", [NativeBackend, PyBackend])
def test_concurrent_status_increments_stale_updates_and_recreates(backend_cls):
    server = InMemoryApiServer(backend=backend_cls())
    owner = server.create({"kind": "RayCluster",
                           "metadata": {"name": "own", "namespace": "d"}})
    ref = [{"kind": "RayCluster", "name": "own", "uid": owner["metadata"]["uid"]}]
    counters = ["ctr-0", "ctr-1"]
    churned = ["tmp-0", "tmp-1", "tmp-2"]
    for name in counters:
        obj = pod(name, ownerReferences=ref)
        obj["status"] = {"phase": "Running", "count": 0}
        server.create(obj)
    done = {name: 0 for name in counters}
    done_lock = threading.Lock()
    problems = []

    def bump(obj):
        obj["status"]["count"] += 1

    def worker(t):
        rng = random.Random(t)
        try:
            for i in range(200):
                kind = i % 4
                if kind in (0, 1):
                    name = rng.choice(counters)
                    if server.mutate_status("Pod", "d", name, bump) is not None:
                        with done_lock:
                            done[name] += 1
                elif kind == 2:
                    cur = server.get("Pod", "d", rng.choice(counters))
                    cur["metadata"]["resourceVersion"] = str(
                        int(cur["metadata"]["resourceVersion"]) - 1)
                    cur["spec"]["restartPolicy"] = "Always"
                    try:
                        server.update(cur)
                        problems.append("stale update went through")
                    except ConflictError:
                        pass
                else:
                    name = rng.choice(churned)
                    try:
                        server.delete("Pod", "d", name)
                    except NotFoundError:
                        pass
                    try:
                        server.create(pod(name, ownerReferences=ref))
                    except AlreadyExistsError:
                        pass
        except Exception as e:  # pragma: no cover
            problems.append(repr(e))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert problems == []
    assert sum(done.values()) == 8 * 100
    for name in counters:
        stored = server.get("Pod", "d", name)
        assert stored["status"]["count"] == done[name]
        assert stored["spec"]["restartPolicy"] == "Never"
    uid = owner["metadata"]["uid"]
    deps = server._backend.dependents(uid)
    assert len(deps) == len(set(deps)) == server.count("Pod")
    assert {d[2] for d in deps} == {o["metadata"]["name"] for o in server.list("Pod")}
    server.delete("RayCluster", "d", "own")
    assert server.count("Pod") == 0 and server.count("RayCluster") == 0
    assert server._backend.dependents(uid) == []
    assert server.list_pod_views() == []
    assert server.kinds() == []
