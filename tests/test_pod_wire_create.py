"""Pods created from wire dicts (RayClusterReconciler._wire_create,
InMemoryClient.create_wire) against the typed path they replace
(KUBERAY_POD_WIRE_CREATE=0): the same stored pods, the same ADDED events,
expectations satisfied, and no typed response built on the way; and the
``discard_result`` form of InMemoryClient.update_status."""
import copy
import itertools
import types

import pytest

from kuberay_amd.kube import objects as k8s
from kuberay_amd.kube import store as store_mod
from kuberay_amd.kube.client import InMemoryClient, KubeClient
from kuberay_amd.kube.objects import K8sModel
from kuberay_amd.kube.store import (ConflictError, InMemoryApiServer,
                                    NotFoundError, PyBackend)
from kuberay_amd.models import RayCluster
from kuberay_amd.ops.raycluster import RayClusterReconciler
from kuberay_amd.parallel.batchscheduler import VolcanoBatchScheduler
from kuberay_amd.testing import simple_raycluster
from kuberay_amd.utils import constants as C

try:
    from kuberay_amd.kube.native import NativeBackend
    BACKENDS = [PyBackend, NativeBackend]
except ImportError:
    BACKENDS = [PyBackend]


@pytest.fixture(autouse=True)
def ids(monkeypatch):
    """uids and timestamps as a pure function of call order."""
    state = types.SimpleNamespace(counter=itertools.count())

    class Uid:
        def __init__(self, n):
            self.hex = f"{n:05x}" + "0" * 27  # generated names take hex[:5]

        def __str__(self):
            return f"uid-{self.hex}"

    monkeypatch.setattr(store_mod, "uuid", types.SimpleNamespace(
        uuid4=lambda: Uid(next(state.counter))))
    monkeypatch.setattr(store_mod, "now_iso", lambda: "2024-06-07T00:00:00Z")
    state.reset = lambda: setattr(state, "counter", itertools.count())
    return state


def cluster_doc(name, replicas=1, num_of_hosts=1, groups=1):
    doc = simple_raycluster(name, workers=replicas, gpus_per_worker=1,
                            num_of_hosts=num_of_hosts).to_dict()
    first = doc["spec"]["workerGroupSpecs"][0]
    for g in range(1, groups):
        other = copy.deepcopy(first)
        other["groupName"] = f"group-{g}"
        other["replicas"] = replicas + g
        other["maxReplicas"] = 8
        doc["spec"]["workerGroupSpecs"].append(other)
    return doc


CASES = {
    "replicas-1": dict(replicas=1),
    "replicas-2": dict(replicas=2),
    "replicas-4": dict(replicas=4),
    "two-groups": dict(replicas=2, groups=2),
    "multi-host": dict(replicas=2, num_of_hosts=2),
}


class FromDictCounter:
    """Counts K8sModel.from_dict calls by model class."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = K8sModel.from_dict.__func__
        counter = self

        def counting(cls, data):
            counter.calls.append(cls.__name__)
            return real(cls, data)

        monkeypatch.setattr(K8sModel, "from_dict", classmethod(counting))

    def of(self, name):
        return sum(1 for c in self.calls if c == name)


def masked(pod):
    """The pod without what differs from run to run: the random name
    suffix (and the replica-group names drawn with it)."""
    pod = copy.deepcopy(pod)
    meta = pod["metadata"]
    assert meta["name"].startswith(meta["generateName"])
    assert len(meta["name"]) == len(meta["generateName"]) + 5
    meta["name"] = meta["generateName"] + "*"
    replica_name = meta["labels"].get(C.RAY_WORKER_REPLICA_NAME_KEY)
    if replica_name:
        meta["labels"][C.RAY_WORKER_REPLICA_NAME_KEY] = \
            replica_name.rsplit("-", 1)[0] + "-*"
        for container in pod["spec"]["containers"]:
            for env in container.get("env") or []:
                if env.get("value") == replica_name:
                    env["value"] = meta["labels"][C.RAY_WORKER_REPLICA_NAME_KEY]
    return pod


def run_once(doc, wire_on, backend_cls, ids, *, client_cls=InMemoryClient,
             batch_scheduler=None):
    ids.reset()
    server = InMemoryApiServer(backend_cls())
    client = client_cls(server)
    reconciler = RayClusterReconciler(client, batch_scheduler=batch_scheduler)
    reconciler.pod_wire_create = wire_on
    watcher = server.watch({"Pod"})
    client.create(RayCluster.from_dict(copy.deepcopy(doc)))
    name = doc["metadata"]["name"]
    reconciler.reconcile(("default", name))
    events = watcher.drain()
    pods = server.list("Pod")
    return types.SimpleNamespace(server=server, reconciler=reconciler,
                                 events=events, pods=pods, name=name)


@pytest.mark.parametrize("backend_cls", BACKENDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_same_pods_and_events_with_the_wire_path_on_and_off(case, backend_cls,
                                                            ids):
    doc = cluster_doc(f"wire-{case}", **CASES[case])
    on = run_once(doc, True, backend_cls, ids)
    off = run_once(doc, False, backend_cls, ids)

    groups = doc["spec"]["workerGroupSpecs"]
    want = 1 + sum(g["replicas"] * g["numOfHosts"] for g in groups)
    assert len(on.pods) == len(off.pods) == want

    # the order of creation is the same, so events pair up one to one
    assert [t for t, _ in on.events] == ["ADDED"] * want
    assert [t for t, _ in off.events] == ["ADDED"] * want
    for (_, a), (_, b) in zip(on.events, off.events):
        assert masked(a) == masked(b)
        assert list(a) == list(b) and list(a["metadata"]) == list(b["metadata"])
    by_rv = lambda pods: sorted(pods, key=lambda p: int(p["metadata"]["resourceVersion"]))
    for a, b in zip(by_rv(on.pods), by_rv(off.pods)):
        assert masked(a) == masked(b)
        assert a["metadata"]["uid"] == b["metadata"]["uid"]
    assert [masked(e) for _, e in on.events] == [masked(p) for p in by_rv(on.pods)]

    # every pod the reconciler said it expects is there
    for run in (on, off):
        for group in ["__head__"] + [g["groupName"] for g in groups]:
            assert run.reconciler.expectations.is_satisfied(
                run.server, "default", run.name, group)
        assert not run.reconciler.expectations._pending


@pytest.mark.parametrize("backend_cls", BACKENDS)
def test_replica_k_is_the_prototype_with_its_index(backend_cls, ids,
                                                   monkeypatch):
    built = []
    real_build = RayClusterReconciler._build_worker_pod

    def recording(self, *args, **kwargs):
        pod = real_build(self, *args, **kwargs)
        built.append(pod.clone())
        return pod

    monkeypatch.setattr(RayClusterReconciler, "_build_worker_pod", recording)
    run = run_once(cluster_doc("wire-proto", replicas=4), True, backend_cls, ids)
    assert len(built) == 1  # one build for the group, three copies of it
    workers = sorted(
        (p for p in run.pods
         if p["metadata"]["labels"][C.RAY_NODE_TYPE_LABEL_KEY] == "worker"),
        key=lambda p: int(p["metadata"]["labels"][C.RAY_WORKER_REPLICA_INDEX_KEY]))
    assert len(workers) == 4
    stamped = ("name", "namespace", "uid", "resourceVersion", "generation",
               "creationTimestamp")
    for k, stored in enumerate(workers):
        expected_pod = built[0].clone()
        expected_pod.metadata.labels[C.RAY_WORKER_REPLICA_INDEX_KEY] = str(k)
        expected = expected_pod.to_dict()
        expected["kind"] = expected_pod.kind
        stored = copy.deepcopy(stored)
        for field in stamped:
            if field not in expected["metadata"]:
                stored["metadata"].pop(field)
        assert stored == expected
        assert list(stored["metadata"]["labels"]) == \
            list(expected["metadata"]["labels"])
    # four names, four uids: the copies are objects of their own
    assert len({p["metadata"]["name"] for p in workers}) == 4
    assert len({p["metadata"]["uid"] for p in workers}) == 4


def test_no_typed_response_is_built_on_the_wire_path(ids, monkeypatch):
    doc = cluster_doc("wire-count", replicas=4)
    counter = FromDictCounter(monkeypatch)
    run_once(doc, True, BACKENDS[-1], ids)
    on = list(counter.calls)
    counter.calls.clear()
    run_once(doc, False, BACKENDS[-1], ids)
    off = list(counter.calls)
    # off: one Pod model per created pod (the response of client.create);
    # on: none. Nothing else changes.
    assert on.count("Pod") == 0
    assert off.count("Pod") == 5
    without_pods = lambda calls: sorted(c for c in calls if c != "Pod")
    assert without_pods(on) == without_pods(off)


class NoWireClient(InMemoryClient):
    create_wire = None  # a client that has no such method to offer


def test_client_without_the_method_takes_the_typed_path(ids, monkeypatch):
    doc = cluster_doc("wire-nowire", replicas=2)
    counter = FromDictCounter(monkeypatch)
    run = run_once(doc, True, BACKENDS[-1], ids, client_cls=NoWireClient)
    assert counter.of("Pod") == 3
    reference = run_once(doc, False, BACKENDS[-1], ids)
    assert [masked(e) for _, e in run.events] == \
        [masked(e) for _, e in reference.events]


def test_batch_scheduler_keeps_the_typed_path(ids, monkeypatch):
    doc = cluster_doc("wire-batch", replicas=3)
    wire_calls = []
    real = InMemoryClient.create_wire

    def counting(self, data):
        wire_calls.append(data["metadata"].get("generateName"))
        return real(self, data)

    monkeypatch.setattr(InMemoryClient, "create_wire", counting)
    counter = FromDictCounter(monkeypatch)
    on = run_once(doc, True, BACKENDS[-1], ids,
                  batch_scheduler=VolcanoBatchScheduler())
    assert wire_calls == []
    assert counter.of("Pod") == 4
    off = run_once(doc, False, BACKENDS[-1], ids,
                   batch_scheduler=VolcanoBatchScheduler())
    assert [masked(e) for _, e in on.events] == [masked(e) for _, e in off.events]
    assert all(p["spec"]["schedulerName"] == "volcano" for p in on.pods)
    # and without one, the same cluster does go the wire way
    run_once(doc, True, BACKENDS[-1], ids)
    assert len(wire_calls) == 4


def test_create_wire_returns_the_stored_dict(ids):
    server = InMemoryApiServer(BACKENDS[-1]())
    client = InMemoryClient(server)
    pod = k8s.Pod.from_dict({
        "metadata": {"generateName": "p-", "namespace": "d",
                     "labels": {"a": "b"}},
        "spec": {"containers": [{"name": "c", "image": "i"}]}})
    data = pod.to_dict()
    data["kind"] = pod.kind
    out = client.create_wire(data)
    assert out is data  # handed over, stamped in place
    assert out["metadata"]["name"].startswith("p-")
    assert server.get("Pod", "d", out["metadata"]["name"]) == out
    typed = client.create(pod)
    stored = server.get("Pod", "d", typed.metadata.name)
    for tree in (stored, out):
        for field in ("name", "uid", "resourceVersion"):
            tree["metadata"].pop(field)
    assert stored == out
    assert not hasattr(KubeClient, "create_wire")


def test_the_switch_is_read_from_the_environment():
    import os
    import subprocess
    import sys
    from pathlib import Path
    code = ("from kuberay_amd.ops.raycluster import RayClusterReconciler as R;"
            "print(R.pod_wire_create)")
    root = Path(__file__).resolve().parent.parent
    for value, want in (("0", "False"), (None, "True")):
        env = {k: v for k, v in os.environ.items()
               if k != "KUBERAY_POD_WIRE_CREATE"}
        if value is not None:
            env["KUBERAY_POD_WIRE_CREATE"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env,
                             capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want


# -- update_status(discard_result=True) --------------------------------------

@pytest.fixture(params=BACKENDS)
def cluster_client(request):
    server = InMemoryApiServer(request.param())
    client = InMemoryClient(server)
    created = client.create(simple_raycluster("st", workers=1))
    return server, client, created


def test_update_status_discarding_returns_none_and_refreshes_rv(cluster_client):
    server, client, cluster = cluster_client
    before = cluster.metadata.resource_version
    cluster.status.state = "ready"
    assert client.update_status(cluster, discard_result=True) is None
    stored = server.get("RayCluster", "default", "st")
    assert stored["status"]["state"] == "ready"
    assert cluster.metadata.resource_version == \
        stored["metadata"]["resourceVersion"] != before
    # the refreshed rv makes the next write go through
    cluster.status.state = "suspended"
    assert client.update_status(cluster, discard_result=True) is None
    assert server.get("RayCluster", "default", "st")["status"]["state"] == \
        "suspended"


def test_update_status_default_form_is_unchanged(cluster_client):
    server, client, cluster = cluster_client
    cluster.status.state = "ready"
    out = client.update_status(cluster)
    assert isinstance(out, RayCluster)
    assert out.status.state == "ready"
    assert out.metadata.resource_version == cluster.metadata.resource_version
    assert out.to_dict() == RayCluster.from_dict(
        server.get("RayCluster", "default", "st")).to_dict()
    out = client.update_status(cluster, discard_result=False)
    assert isinstance(out, RayCluster)


def test_update_status_discarding_raises_the_same_errors(cluster_client):
    server, client, cluster = cluster_client
    stale = cluster.clone()
    cluster.status.state = "ready"
    client.update_status(cluster, discard_result=True)
    for discard in (True, False):
        with pytest.raises(ConflictError):
            client.update_status(stale.clone(), discard_result=discard)
    server.delete("RayCluster", "default", "st")
    for discard in (True, False):
        with pytest.raises(NotFoundError):
            client.update_status(cluster.clone(), discard_result=discard)


def test_reconciler_discards_only_where_the_client_can(ids, monkeypatch):
    doc = cluster_doc("st-rec", replicas=1)
    counter = FromDictCounter(monkeypatch)
    run_once(doc, True, BACKENDS[-1], ids)
    with_discard = counter.of("RayCluster")
    counter.calls.clear()

    class PlainStatusClient(InMemoryClient):
        def update_status(self, obj):  # the KubeClient signature, no keyword
            return super().update_status(obj)

    run = run_once(doc, True, BACKENDS[-1], ids, client_cls=PlainStatusClient)
    assert run.reconciler._status_kwargs == {}
    # the one status write of this reconcile built a model there, none here
    assert counter.of("RayCluster") == with_discard + 1
