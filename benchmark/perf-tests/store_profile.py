#!/usr/bin/env python3
"""Where the control plane's CPU goes, per call site: the object store, and
above it the model copies, the typed gets by kind and the RayCluster
reconciler's steps.

Runs N bench-style steps (bench.py's run_step: create the RayClusters, wait
for Ready, delete, drain) with those entry points and the store's JSON calls
wrapped in ``time.thread_time()`` and prints each site's share of the
process CPU. The benchmark is one GIL-bound core of host work (the GPU idles
during it), so this table — not a kernel profile — is what says where a
store change pays.

    python benchmark/perf-tests/store_profile.py --clusters 200 --steps 3

``--micro`` instead times one stored object three ways, for the bench's
worker pod, head pod and RayCluster: the engine's decode from the stored
sections, blob assembly + ``json.loads``, and ``engine.copy_tree`` of the
parsed tree (the cost of creating the containers alone, the decoder's floor).

``--root DIR`` profiles another checkout of this repository (for a
before/after on the same host); every site is looked up by name and skipped
where a checkout does not have it. CPU-only: no GPU is touched.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time
from collections import defaultdict


class Sites:
    """Per-site thread-CPU accumulators (inclusive time)."""

    def __init__(self) -> None:
        self.cpu = defaultdict(float)
        self.calls = defaultdict(int)
        self.lock = threading.Lock()
        self.tls = threading.local()

    def add(self, site: str, dt: float) -> None:
        with self.lock:
            self.cpu[site] += dt
            self.calls[site] += 1

    def wrap(self, site: str, fn, group: str = None):
        """Time ``fn`` under ``site``; with ``group``, the outermost call of
        any function of that group is also charged to the group (nested
        calls, e.g. update() inside mutate_status(), are not counted twice)."""
        sites = self
        clock = time.thread_time

        def timed(*args, **kwargs):
            tls = sites.tls
            depth = getattr(tls, "depth", None)
            if depth is None:
                depth = tls.depth = defaultdict(int)
            outer = group is not None and depth[group] == 0
            if group is not None:
                depth[group] += 1
            t0 = clock()
            try:
                return fn(*args, **kwargs)
            finally:
                dt = clock() - t0
                if group is not None:
                    depth[group] -= 1
                sites.add(site, dt)
                if outer:
                    sites.add(group, dt)
        timed.__wrapped__ = fn
        return timed


STORE_VERBS = ("create", "update", "delete", "get", "try_get", "list",
               "list_pod_views", "patch_merge", "mutate_status",
               "events_since")


def instrument(sites: Sites) -> None:
    from kuberay_amd.kube import store as store_mod
    server_cls = store_mod.InMemoryApiServer
    for verb in STORE_VERBS:
        fn = getattr(server_cls, verb, None)
        if fn is not None:
            setattr(server_cls, verb, sites.wrap(
                f"InMemoryApiServer.{verb}", fn, group="store layer (all verbs)"))

    # the watch-history serialization happens inside _notify through the
    # json module itself; tell it apart from every other json.dumps caller
    notify = server_cls._notify
    real_dumps = json.dumps
    timed_hist = sites.wrap("json.dumps in _notify (watch history)", real_dumps)
    timed_other = sites.wrap("json.dumps elsewhere", real_dumps)

    def dumps(*args, **kwargs):
        if getattr(sites.tls, "in_notify", 0):
            return timed_hist(*args, **kwargs)
        return timed_other(*args, **kwargs)

    def notify_flagged(self, *args, **kwargs):
        sites.tls.in_notify = getattr(sites.tls, "in_notify", 0) + 1
        try:
            return notify(self, *args, **kwargs)
        finally:
            sites.tls.in_notify -= 1

    try:
        from kuberay_amd.kube import native as native_mod
    except ImportError:
        native_mod = None
    # native.py binds json.dumps / json.loads at import: wrap its own names
    # before json.dumps is replaced below
    if native_mod is not None:
        native_mod._loads = sites.wrap(
            "json.loads of stored blobs (NativeBackend)", native_mod._loads)
        native_mod._dumps = sites.wrap(
            "json.dumps in NativeBackend.put", native_mod._dumps)
        backend_cls = native_mod.NativeBackend
        for name in ("put", "put_status", "fetch", "remove", "list",
                     "list_views", "peek", "history_since"):
            fn = getattr(backend_cls, name, None)
            if fn is not None:
                setattr(backend_cls, name,
                        sites.wrap(f"NativeBackend.{name}", fn))
        # the reads themselves, inside the engine: trees decoded from the
        # sections, or blobs assembled for json.loads (the row above)
        store_cls = getattr(native_mod.engine, "NativeStore", None)
        for site, names in (
                ("native decode of stored objects (NativeStore.*_tree[s])",
                 ("fetch_tree", "remove_tree", "list_trees",
                  "history_since_trees")),
                ("blob assembly for json.loads (NativeStore reads)",
                 ("fetch", "remove", "list_blobs", "history_since"))):
            for name in names:
                fn = getattr(store_cls, name, None)
                if fn is not None:
                    setattr(store_cls, name, sites.wrap(site, fn))
    json.dumps = dumps
    server_cls._notify = sites.wrap("InMemoryApiServer._notify", notify_flagged)


RECONCILER_SITES = ("reconcile", "_create_head_pod", "_create_worker_pod",
                    "_calculate_and_update_status", "_reconcile_head_service",
                    "_update_endpoints", "_update_head_info")


def instrument_reconciler(sites: Sites) -> None:
    """The call sites above the store: model copies, typed gets by kind and
    the RayCluster reconciler's steps (inclusive times; reconcile contains
    the others)."""
    from kuberay_amd.kube import client as client_mod
    from kuberay_amd.kube import objects as objects_mod
    from kuberay_amd.ops import raycluster as rc_mod

    objects_mod.K8sModel.clone = sites.wrap(
        "K8sModel.clone", objects_mod.K8sModel.clone)

    objects_mod.K8sModel.to_dict = sites.wrap(
        "K8sModel.to_dict", objects_mod.K8sModel.to_dict)
    objects_mod.K8sModel.from_dict = classmethod(sites.wrap(
        "K8sModel.from_dict", objects_mod.K8sModel.from_dict.__func__))
    create_wire = getattr(client_mod.InMemoryClient, "create_wire", None)
    if create_wire is not None:
        client_mod.InMemoryClient.create_wire = sites.wrap(
            "client.create_wire (pods as wire dicts)", create_wire)
    client_mod.InMemoryClient.create = sites.wrap(
        "client.create (typed)", client_mod.InMemoryClient.create)

    real_get = client_mod.InMemoryClient.get
    clock = time.thread_time

    def get(self, model, namespace, name):
        t0 = clock()
        try:
            return real_get(self, model, namespace, name)
        finally:
            sites.add(f"client.get({getattr(model, '__name__', model)})",
                      clock() - t0)
    client_mod.InMemoryClient.get = get

    cls = rc_mod.RayClusterReconciler
    for name in RECONCILER_SITES:
        fn = getattr(cls, name, None)
        if fn is not None:
            setattr(cls, name, sites.wrap(f"RayClusterReconciler.{name}", fn))


def micro() -> int:
    """One bench cluster brought to Ready, then per object: decode from the
    sections, blob + json.loads and copy_tree, best of five timed loops."""
    from kuberay_amd._native import engine
    from kuberay_amd.testing import ControlPlane, simple_raycluster

    cp = ControlPlane(kubelet_delay=0.0, workers=2, record_events=False,
                      requeue_seconds=3600, poll_seconds=1.0,
                      kubelet_executors=2)
    cp.start()
    try:
        name = "bench-r0-s0-0000"
        cp.client.create(simple_raycluster(name, workers=3, gpus_per_worker=1))
        if not cp.wait_cluster_state("default", name, "ready", timeout=60):
            raise RuntimeError("cluster never became ready")
        store = cp.server._backend._store
        pods = [p["metadata"]["name"] for p in cp.server.list("Pod")]
        subjects = [
            ("worker pod", "Pod", next(n for n in pods if "worker" in n)),
            ("head pod", "Pod", next(n for n in pods if "head" in n)),
            ("RayCluster", "RayCluster", name)]

        def best_us(fn, loops=5000):
            best = float("inf")
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(loops):
                    fn()
                best = min(best, (time.perf_counter() - t0) / loops)
            return best * 1e6

        print("| object | bytes | native decode us | blob + json.loads us | "
              "ratio | copy_tree us |")
        print("|---|---|---|---|---|---|")
        for label, kind, obj_name in subjects:
            key = (kind, "default", obj_name)
            blob = store.fetch(*key)
            tree = json.loads(blob)
            decoded = store.fetch_tree(*key)
            if type(decoded) is not dict or decoded != tree:
                raise RuntimeError(f"{label}: decoder fell back or differs")
            t_dec = best_us(lambda: store.fetch_tree(*key))
            t_loads = best_us(lambda: json.loads(store.fetch(*key)))
            t_copy = best_us(lambda: engine.copy_tree(tree))
            print(f"| {label} | {len(blob)} | {t_dec:.1f} | {t_loads:.1f} | "
                  f"{t_loads / t_dec:.2f}x | {t_copy:.1f} |")
    finally:
        cp.stop()
    return 0


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--clusters", type=int, default=200)
    parser.add_argument("--steps", type=int, default=3)
    parser.add_argument("--warmup", type=int, default=1)
    parser.add_argument("--workers-per-cluster", type=int, default=3)
    parser.add_argument("--controller-workers", type=int, default=4)
    parser.add_argument("--root", default=None,
                        help="checkout to profile (default: this one)")
    parser.add_argument("--json", action="store_true",
                        help="print the table as one JSON line as well")
    parser.add_argument("--micro", action="store_true",
                        help="time decode / json.loads / copy_tree of the "
                             "bench objects instead of profiling steps")
    args = parser.parse_args()

    root = os.path.abspath(args.root or os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    sys.path.insert(0, root)
    if args.micro:
        return micro()
    import bench  # the checkout's own step definition
    from kuberay_amd.testing import ControlPlane

    sites = Sites()
    instrument(sites)
    instrument_reconciler(sites)

    cp = ControlPlane(kubelet_delay=0.0, workers=args.controller_workers,
                      record_events=False, requeue_seconds=3600,
                      poll_seconds=1.0, kubelet_executors=2)
    cp.start()
    try:
        for w in range(args.warmup):
            bench.run_step(cp, args.clusters, args.workers_per_cluster, 1,
                           step_idx=-1 - w, rank=0)
        with sites.lock:
            sites.cpu.clear()
            sites.calls.clear()
        cpu0, wall0 = time.process_time(), time.perf_counter()
        for k in range(args.steps):
            bench.run_step(cp, args.clusters, args.workers_per_cluster, 1,
                           step_idx=k, rank=0)
        cpu, wall = time.process_time() - cpu0, time.perf_counter() - wall0
        stats = getattr(cp.server._backend, "stats", None)
        engine_stats = stats() if stats else None
        try:
            from kuberay_amd._native import engine
            copy_stats = engine.copy_stats()
        except (ImportError, AttributeError):
            copy_stats = None
    finally:
        cp.stop()

    with sites.lock:
        snapshot = {s: (sites.cpu[s], sites.calls[s]) for s in sites.cpu}
    put = snapshot.get("NativeBackend.put")
    if put:
        inner = snapshot.get("json.dumps in NativeBackend.put", (0.0, 0))
        snapshot["NativeBackend.put minus its json.dumps"] = (
            put[0] - inner[0], put[1])

    total_clusters = args.clusters * args.steps
    print(f"root: {root}")
    print(f"backend: {cp.server.backend_name}   clusters/step: {args.clusters}"
          f"   steps: {args.steps}")
    print(f"wall {wall:.2f} s   process CPU {cpu:.2f} s   "
          f"{total_clusters / wall:.1f} clusters/s   "
          f"{cpu / total_clusters * 1e3:.2f} ms CPU/cluster")
    print()
    print(f"| {'where':<52} | {'share':>6} | {'calls':>7} | {'CPU s':>7} | "
          f"{'us/call':>7} |")
    print(f"|{'-' * 54}|{'-' * 8}|{'-' * 9}|{'-' * 9}|{'-' * 9}|")
    for site, (t, n) in sorted(snapshot.items(), key=lambda kv: -kv[1][0]):
        print(f"| {site:<52} | {100 * t / cpu:5.1f}% | {n:7d} | {t:7.3f} | "
              f"{(t / n * 1e6 if n else 0):7.1f} |")
    if engine_stats:
        print()
        print("engine counters (whole run, warm-up included): "
              + ", ".join(f"{k}={v}" for k, v in engine_stats.items()))
    if copy_stats:
        print("tree copier (whole run, warm-up included): "
              + ", ".join(f"{k}={v}" for k, v in copy_stats.items()))
    if args.json:
        print(json.dumps({
            "root": root, "wall_s": wall, "cpu_s": cpu,
            "clusters_per_s": total_clusters / wall,
            "sites": {s: {"cpu_s": t, "calls": n, "share": t / cpu}
                      for s, (t, n) in snapshot.items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
