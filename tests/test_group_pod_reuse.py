"""One build per worker-group scale-up: the pods stored with the reuse on are
the pods stored with it off, replica by replica, whatever the spec carries;
build_pod runs once per group per reconcile instead of once per pod; multi-host
groups do not take the path."""
import glob
import json
import os

import pytest
import yaml

import kuberay_amd.features as features
from kuberay_amd.common import pod as podlib
from kuberay_amd.kube import objects as k8s
from kuberay_amd.kube.client import InMemoryClient
from kuberay_amd.kube.store import InMemoryApiServer
from kuberay_amd.models import RayCluster, RayNodeType
from kuberay_amd.ops.raycluster import (RayClusterReconciler,
                                        RayClusterReconcilerOptions)
from kuberay_amd.parallel.batchscheduler import (VolcanoBatchScheduler,
                                                 XgmiGangScheduler,
                                                 YunikornBatchScheduler)
from kuberay_amd.testing import simple_raycluster
from kuberay_amd.utils import constants as C

SAMPLES_DIR = os.path.join(os.path.dirname(__file__), "..", "deploy", "samples")
GATES = ("RayClusterMTLS", "RayClusterNetworkPolicy", "RayClusterHistoryServer",
         "GCSFaultToleranceEmbeddedStorage", "RayCronJob")


@pytest.fixture(autouse=True)
def _gates():
    for g in GATES:
        features.set_gate(g, True)
    yield
    features.reset()


def _sample_clusters():
    out = []
    for path in sorted(glob.glob(os.path.join(SAMPLES_DIR, "*.yaml"))):
        with open(path) as f:
            for doc in yaml.safe_load_all(f):
                if doc and doc.get("kind") == "RayCluster":
                    out.append((os.path.basename(path), doc))
    return out


def _sidecar_options():
    options = RayClusterReconcilerOptions()
    options.worker_sidecar_containers = [k8s.Container(
        name="log-shipper", image="fluent-bit",
        env=[k8s.EnvVar(name="A", value="b")],
        volume_mounts=[k8s.VolumeMount(name="logs", mount_path="/logs")])]
    options.default_container_envs = [k8s.EnvVar(name="SITE", value="lab")]
    return options


def _burn_in():
    cluster = simple_raycluster("demo", workers=1, gpus_per_worker=8)
    cluster.spec.worker_group_specs[0].template.metadata.annotations = {
        C.GPU_BURN_IN_ANNOTATION_KEY: "true"}
    return cluster


def _two_groups():
    cluster = simple_raycluster("demo", workers=1, gpus_per_worker=1)
    second = cluster.spec.worker_group_specs[0].clone()
    second.group_name = "second-group"
    second.resources = {"custom": "2"}
    second.labels = {"tier": "b"}
    cluster.spec.worker_group_specs.append(second)
    return cluster


# name -> (cluster as a dict, reconciler keyword arguments)
def _variants():
    out = {}
    for fname, doc in _sample_clusters():
        out["sample:" + fname] = (doc, {})
    out["plain"] = (simple_raycluster("demo", gpus_per_worker=1).to_dict(), {})
    out["two-groups"] = (_two_groups().to_dict(), {})
    out["sidecars"] = (simple_raycluster("demo").to_dict(),
                       {"options": _sidecar_options})
    out["autoscaler-v2"] = (simple_raycluster(
        "demo", enableInTreeAutoscaling=True,
        autoscalerOptions={"version": "v2"}).to_dict(), {})
    out["auth"] = (simple_raycluster(
        "demo", rayVersion="2.52.0", authOptions={"mode": "token"}).to_dict(), {})
    out["burn-in"] = (_burn_in().to_dict(), {})
    out["volcano"] = (simple_raycluster("demo").to_dict(),
                      {"batch_scheduler": VolcanoBatchScheduler})
    out["yunikorn"] = (simple_raycluster("demo").to_dict(),
                       {"batch_scheduler": YunikornBatchScheduler})
    # appends to the pod's affinity every time it is handed one
    out["xgmi-gang"] = (simple_raycluster("demo", gpus_per_worker=1).to_dict(),
                        {"batch_scheduler": XgmiGangScheduler})
    return out


VARIANTS = _variants()
SINGLE_HOST = [n for n, (doc, _) in VARIANTS.items()
               if all((g.get("numOfHosts") or 1) == 1
                      for g in doc["spec"].get("workerGroupSpecs") or [])
               and doc["spec"].get("workerGroupSpecs")]


class BuildCounter:
    """Counts build_pod calls for workers, per reconcile."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = podlib.build_pod

        def counting(template, node_type, *args, **kwargs):
            if node_type == RayNodeType.WORKER:
                self.calls.append(
                    template.metadata.labels[C.RAY_NODE_GROUP_LABEL_KEY])
            return real(template, node_type, *args, **kwargs)
        monkeypatch.setattr(podlib, "build_pod", counting)


def _scale_up(doc, replicas, reuse, reconciler_kwargs, counter):
    """Create the cluster with `replicas` per group and reconcile once: the
    head pod and every worker pod are created by that one pass."""
    server = InMemoryApiServer()
    client = InMemoryClient(server)
    kwargs = {k: make() for k, make in reconciler_kwargs.items()}
    reconciler = RayClusterReconciler(client, **kwargs)
    reconciler.group_pod_reuse = reuse
    cluster = RayCluster.from_dict(doc)
    for g in cluster.spec.worker_group_specs:
        g.replicas = replicas
        g.min_replicas = 0
        g.max_replicas = max(replicas, g.max_replicas or 0)
    client.create(cluster)
    del counter.calls[:]
    reconciler.reconcile(("default", cluster.metadata.name))
    built = list(counter.calls)
    pods = [p for p in server.list("Pod")
            if p["metadata"]["labels"][C.RAY_NODE_TYPE_LABEL_KEY] == "worker"]
    # the owner is a cluster created anew for each run; its uid is in the
    # owner reference and, with GCS fault tolerance, in an annotation
    uid = server.get("RayCluster", "default", cluster.metadata.name)["metadata"]["uid"]
    pods = json.loads(json.dumps(pods).replace(uid, "CLUSTER-UID"))
    return cluster, pods, built, reconciler


def _normalized(pods):
    out = []
    for p in pods:
        meta = dict(p["metadata"])
        for k in ("name", "uid", "resourceVersion", "creationTimestamp"):
            assert meta.pop(k, None), k
        out.append(dict(p, metadata=meta))
    out.sort(key=lambda p: (p["metadata"]["labels"][C.RAY_NODE_GROUP_LABEL_KEY],
                            int(p["metadata"]["labels"][C.RAY_WORKER_REPLICA_INDEX_KEY])))
    return out


@pytest.mark.parametrize("replicas", [1, 2, 3])
@pytest.mark.parametrize("variant", SINGLE_HOST)
def test_stored_pods_are_the_same_with_reuse_on_and_off(variant, replicas,
                                                        monkeypatch):
    doc, reconciler_kwargs = VARIANTS[variant]
    counter = BuildCounter(monkeypatch)
    cluster, pods_on, built_on, rec_on = _scale_up(
        doc, replicas, True, reconciler_kwargs, counter)
    _, pods_off, built_off, rec_off = _scale_up(
        doc, replicas, False, reconciler_kwargs, counter)
    groups = [g.group_name for g in cluster.spec.worker_group_specs]

    assert len(pods_on) == len(pods_off) == replicas * len(groups)
    on, off = _normalized(pods_on), _normalized(pods_off)
    assert on == off
    for g in groups:
        indexes = [p["metadata"]["labels"][C.RAY_WORKER_REPLICA_INDEX_KEY]
                   for p in on
                   if p["metadata"]["labels"][C.RAY_NODE_GROUP_LABEL_KEY] == g]
        assert indexes == [str(i) for i in range(replicas)]
    # names come from the store: all different
    assert len({p["metadata"]["name"] for p in pods_on}) == len(pods_on)
    # one build per group with the reuse, one per pod without
    assert sorted(built_on) == sorted(groups)
    assert sorted(built_off) == sorted(groups * replicas)
    # every pod is expected, one by one, either way
    for rec in (rec_on, rec_off):
        for g in groups:
            assert not rec.expectations.is_satisfied(
                InMemoryApiServer(), "default", cluster.metadata.name, g)


@pytest.mark.parametrize("variant", ["plain", "xgmi-gang"])
def test_one_event_per_created_pod(variant, monkeypatch):
    doc, reconciler_kwargs = VARIANTS[variant]
    counter = BuildCounter(monkeypatch)
    seen = {}
    for reuse in (True, False):
        server = InMemoryApiServer()
        client = InMemoryClient(server)
        from kuberay_amd.kube.events import StoreRecorder
        kwargs = {k: make() for k, make in reconciler_kwargs.items()}
        rec = RayClusterReconciler(client, recorder=StoreRecorder(server), **kwargs)
        rec.group_pod_reuse = reuse
        cluster = RayCluster.from_dict(doc)
        cluster.spec.worker_group_specs[0].replicas = 3
        client.create(cluster)
        rec.reconcile(("default", cluster.metadata.name))
        pod_names = {p["metadata"]["name"] for p in server.list("Pod")
                     if p["metadata"]["labels"][C.RAY_NODE_TYPE_LABEL_KEY] == "worker"}
        created = [e for e in server.list("Event")
                   if e.get("reason") == "CreatedWorkerPod"]
        assert len(pod_names) == 3
        assert sum(e.get("count") or 1 for e in created) == 3
        seen[reuse] = sorted((e.get("type"), e.get("count")) for e in created)
    assert seen[True] == seen[False]


def test_later_scale_up_continues_the_indexes(monkeypatch):
    counter = BuildCounter(monkeypatch)
    server = InMemoryApiServer()
    client = InMemoryClient(server)
    rec = RayClusterReconciler(client)
    rec.group_pod_reuse = True
    client.create(simple_raycluster("demo", workers=1))
    rec.reconcile(("default", "demo"))
    assert counter.calls == ["default-group"]
    cluster = client.get(RayCluster, "default", "demo")
    cluster.spec.worker_group_specs[0].replicas = 4
    client.update(cluster)
    # the pods of the first pass are in the store, so expectations are met
    del counter.calls[:]
    rec.reconcile(("default", "demo"))
    assert counter.calls == ["default-group"]
    labels = sorted(p["metadata"]["labels"][C.RAY_WORKER_REPLICA_INDEX_KEY]
                    for p in server.list("Pod")
                    if p["metadata"]["labels"][C.RAY_NODE_TYPE_LABEL_KEY] == "worker")
    assert labels == ["0", "1", "2", "3"]


def test_multihost_group_does_not_take_the_reuse_path(monkeypatch):
    counter = BuildCounter(monkeypatch)
    doc = simple_raycluster("demo", workers=2, num_of_hosts=3).to_dict()
    _, pods, built, _ = _scale_up(doc, 2, True, {}, counter)
    assert len(pods) == 6
    assert built == ["default-group"] * 6
    hosts = sorted((p["metadata"]["labels"][C.RAY_WORKER_REPLICA_INDEX_KEY],
                    p["metadata"]["labels"][C.RAY_HOST_INDEX_KEY]) for p in pods)
    assert hosts == [(str(r), str(h)) for r in range(2) for h in range(3)]
    # and the sample that has one
    multihost = [doc for f, doc in _sample_clusters() if "multihost" in f]
    assert multihost
    cluster, pods, built, _ = _scale_up(multihost[0], 2, True, {}, counter)
    per_group = {g.group_name: max(g.num_of_hosts, 1) * 2
                 for g in cluster.spec.worker_group_specs}
    assert len(pods) == sum(per_group.values())
    for g, n in per_group.items():
        want = n if n > 2 else 1  # single-host groups of the sample do reuse
        assert built.count(g) == want


@pytest.mark.parametrize("reuse", [True, False])
def test_ray_start_params_defaulting_stays_visible_on_the_group(reuse):
    server = InMemoryApiServer()
    client = InMemoryClient(server)
    rec = RayClusterReconciler(client)
    rec.group_pod_reuse = reuse
    cluster = _two_groups()
    for g in cluster.spec.worker_group_specs:
        g.replicas = 3
    cluster = client.create(cluster)
    group = cluster.spec.worker_group_specs[1]
    assert "resources" not in group.ray_start_params
    assert rec._reconcile_worker_group(cluster, group, []) is True
    assert group.ray_start_params["resources"] == "'{\"custom\": 2.0}'"
    assert group.ray_start_params["labels"] == "'{\"tier\": \"b\"}'"
    pods = server.list("Pod")
    assert len(pods) == 3
    for p in pods:
        args = p["spec"]["containers"][0]["args"][0]
        assert "--resources=" in args and "custom" in args
