"""Service views: the engine's view equals compute_service_view on every
shape, follows the object through its life on both backends, is never wrong
(an unexpected shape gives no view, not a guess), and the RayCluster status
the reconciler publishes from it is the one it publishes from the typed
Service."""
import pytest

from kuberay_amd.kube import objects as k8s
from kuberay_amd.kube.client import InMemoryClient
from kuberay_amd.kube.snapshot import load_snapshot, save_snapshot
from kuberay_amd.kube.store import (InMemoryApiServer, PyBackend, ServiceView,
                                    compute_service_view)
from kuberay_amd.models import RayCluster
from kuberay_amd.ops.raycluster import RayClusterReconciler
from kuberay_amd.testing import simple_raycluster
from kuberay_amd.utils import constants as C
from kuberay_amd.utils import names

try:
    from kuberay_amd.kube.native import NativeBackend
except ImportError:
    NativeBackend = None

BACKENDS = [pytest.param(PyBackend, id="python")]
if NativeBackend is not None:
    BACKENDS.append(pytest.param(NativeBackend, id="native"))
needs_native = pytest.mark.skipif(NativeBackend is None,
                                  reason="native engine not built")


def svc(name="s", namespace="default", **top):
    obj = {"apiVersion": "v1", "kind": "Service",
           "metadata": {"name": name, "namespace": namespace,
                        "resourceVersion": "1", "uid": "u-" + name}}
    obj.update(top)
    return obj


PORTS = [{"name": "gcs", "port": 6379, "targetPort": 6379},
         {"name": "dashboard", "port": 8265}]

# (id, object, has a view)
SHAPES = [
    ("no-spec", svc(), True),
    ("no-ports", svc(spec={"clusterIP": "10.0.0.1", "selector": {"a": "b"}}), True),
    ("ports-null", svc(spec={"ports": None, "clusterIP": None}), True),
    ("empty-ports", svc(spec={"ports": []}), True),
    ("named-ports", svc(spec={"clusterIP": "10.0.0.2", "ports": PORTS}), True),
    ("unnamed-ports", svc(spec={"ports": [{"port": 80}, {"name": None, "port": 81},
                                          {"name": "", "port": 82}]}), True),
    ("node-port", svc(spec={"type": "NodePort", "clusterIP": "10.0.0.3", "ports": [
        {"name": "a", "port": 80, "nodePort": 30080},
        {"name": "b", "port": 81, "nodePort": 0},
        {"name": "c", "port": 82, "nodePort": None}]}), True),
    ("headless", svc(spec={"clusterIP": "None", "ports": PORTS}), True),
    ("port-without-number", svc(spec={"ports": [{"name": "x"}]}), True),
    ("no-namespace", {"kind": "Service", "metadata": {"name": "s"},
                      "spec": {"ports": PORTS}}, True),
    ("unicode", svc(name="s", spec={"ports": [{"name": "pé中", "port": 1}]}), True),
    ("negative-and-large", svc(spec={"ports": [
        {"name": "n", "port": -1, "nodePort": 2 ** 63 - 1}]}), True),
    # no view: the typed path decides what these mean
    ("str-port", svc(spec={"ports": [{"name": "a", "port": "80"}]}), False),
    ("bool-port", svc(spec={"ports": [{"name": "a", "port": True}]}), False),
    ("float-port", svc(spec={"ports": [{"name": "a", "port": 80.0}]}), False),
    ("huge-port", svc(spec={"ports": [{"name": "a", "port": 2 ** 63}]}), False),
    ("str-node-port", svc(spec={"ports": [{"name": "a", "port": 1,
                                           "nodePort": "30000"}]}), False),
    ("int-name", svc(spec={"ports": [{"name": 5, "port": 1}]}), False),
    ("port-not-a-dict", svc(spec={"ports": ["80"]}), False),
    ("ports-not-a-list", svc(spec={"ports": {"a": 1}}), False),
    ("spec-null", svc(spec=None), False),
    ("spec-not-a-dict", svc(spec=[]), False),
    ("int-cluster-ip", svc(spec={"clusterIP": 5}), False),
    ("empty-cluster-ip", svc(spec={"clusterIP": ""}), False),
    ("second-port-bad", svc(spec={"ports": [{"name": "ok", "port": 1},
                                            {"name": "bad", "port": "2"}]}), False),
]


def key_of(obj):
    return ("Service", obj["metadata"].get("namespace", "default"),
            obj["metadata"]["name"])


@pytest.mark.parametrize("backend_cls", BACKENDS)
@pytest.mark.parametrize("name,obj,has_view", SHAPES, ids=[s[0] for s in SHAPES])
def test_backend_view_equals_compute_service_view(backend_cls, name, obj, has_view):
    want = compute_service_view(obj)
    assert (want is not None) == has_view
    backend = backend_cls()
    backend.put(key_of(obj), obj)
    got = backend.service_view(key_of(obj))
    assert got == want
    if backend_cls is not PyBackend:
        # the engine took the tree itself, so this is its own extraction
        # (but for the int its encoder leaves to json.dumps)
        assert backend.stats()["fallbacks"] == (1 if name == "huge-port" else 0)
    if want is not None:
        assert isinstance(got, ServiceView)
        assert all(type(p) is tuple and len(p) == 3 for p in got.ports)


VIEWED = [(s[0], s[1]) for s in SHAPES if s[2]]


@pytest.mark.parametrize("name,obj", VIEWED, ids=[s[0] for s in VIEWED])
def test_view_says_what_the_typed_service_says(name, obj):
    """The two readers in the reconciler, on the view and on the typed
    object."""
    view = compute_service_view(obj)
    typed = k8s.Service.from_dict(obj)
    typed_endpoints = {p.name: str(p.node_port or p.port)
                       for p in typed.spec.ports or [] if p.name}
    view_endpoints = {n: str(node_port or port)
                      for n, port, node_port in view.ports if n}
    assert view_endpoints == typed_endpoints
    assert view.name == typed.metadata.name
    assert (view.cluster_ip or None) == typed.spec.cluster_ip


@needs_native
def test_tree_the_encoder_declines_takes_the_blob_path():
    obj = svc(spec={"clusterIP": "10.0.0.9", "ports": PORTS},
              extra={"a tuple": (1, 2)})
    backend = NativeBackend()
    backend.put(key_of(obj), obj)
    assert backend.stats()["fallbacks"] == 1
    assert backend.service_view(key_of(obj)) == compute_service_view(obj)
    assert backend.service_view(key_of(obj)).ports == [
        ("gcs", 6379, None), ("dashboard", 8265, None)]
    # and a shape without a view stays without one on that path
    bad = svc(name="bad", spec={"ports": [{"name": "a", "port": "80"}]},
              extra={"a tuple": (1, 2)})
    backend.put(key_of(bad), bad)
    assert backend.stats()["fallbacks"] == 2
    assert backend.service_view(key_of(bad)) is None
    assert backend.contains(key_of(bad))


@pytest.mark.parametrize("backend_cls", BACKENDS)
def test_only_services_have_service_views(backend_cls):
    backend = backend_cls()
    pod = {"kind": "Pod", "metadata": {"name": "s", "namespace": "default",
                                       "resourceVersion": "1"},
           "spec": {"clusterIP": "1.1.1.1", "ports": PORTS}}
    backend.put(("Pod", "default", "s"), pod)
    assert backend.service_view(("Service", "default", "s")) is None


@pytest.mark.parametrize("backend_cls", BACKENDS)
def test_lifecycle(backend_cls, tmp_path):
    server = InMemoryApiServer(backend_cls())
    assert server.service_view("default", "s") is None
    created = server.create({"kind": "Service", "metadata": {"name": "s"},
                             "spec": {"clusterIP": "10.0.0.1", "ports": PORTS}})
    first = server.service_view("default", "s")
    assert first == ServiceView("s", "default", "10.0.0.1",
                                [("gcs", 6379, None), ("dashboard", 8265, None)])
    assert server.service_view("other", "s") is None

    # a spec update that changes ports
    created["spec"]["ports"] = [{"name": "gcs", "port": 6380, "nodePort": 31000}]
    updated = server.update(created)
    assert server.service_view("default", "s").ports == [("gcs", 6380, 31000)]

    # a status write keeps the view, and so does a status patch
    updated["status"] = {"loadBalancer": {"ingress": [{"ip": "1.2.3.4"}]}}
    server.update(updated, subresource="status")
    assert server.get("Service", "default", "s")["status"]["loadBalancer"]
    assert server.service_view("default", "s") == ServiceView(
        "s", "default", "10.0.0.1", [("gcs", 6380, 31000)])
    server.patch_merge("Service", "default", "s", {"status": {"x": 1}},
                       subresource="status")
    assert server.service_view("default", "s").ports == [("gcs", 6380, 31000)]

    # an update into a shape without a view drops the old view
    current = server.get("Service", "default", "s")
    current["spec"]["ports"] = [{"name": "gcs", "port": "6380"}]
    server.update(current)
    assert server.service_view("default", "s") is None
    current = server.get("Service", "default", "s")
    current["spec"]["ports"] = [{"name": "gcs", "port": 6381}]
    server.update(current)
    assert server.service_view("default", "s").ports == [("gcs", 6381, None)]

    # snapshot restore
    path = str(tmp_path / "snap.jsonl")
    assert save_snapshot(server, path) == 1
    restored = InMemoryApiServer(backend_cls())
    assert load_snapshot(restored, path) == 1
    assert restored.service_view("default", "s") == server.service_view("default", "s")

    # delete
    server.delete("Service", "default", "s")
    assert server.service_view("default", "s") is None
    assert restored.service_view("default", "s") is not None


def test_server_without_backend_views_answers_none():
    class Bare(PyBackend):
        service_view = None

    server = InMemoryApiServer(Bare())
    server.create({"kind": "Service", "metadata": {"name": "s"}, "spec": {}})
    assert server.service_view("default", "s") is None


# ---------------------------------------------------------------------------
# the reconciler: same status with the views on and off
# ---------------------------------------------------------------------------

class CountingClient(InMemoryClient):
    def __init__(self, server):
        super().__init__(server)
        self.service_gets = 0

    def get(self, model, namespace, name):
        if model is k8s.Service:
            self.service_gets += 1
        return super().get(model, namespace, name)


class NoViewClient(CountingClient):
    service_view = None  # a client that has no such method to offer


def _start_pods(server):
    """What a kubelet does, with addresses that do not depend on timing."""
    pods = server.list("Pod")
    for pod in pods:
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


def _published_status(views_on, backend_cls, *, cluster=None, before=None,
                      between=None, client_cls=CountingClient):
    server = InMemoryApiServer(backend_cls())
    client = client_cls(server)
    reconciler = RayClusterReconciler(client)
    reconciler.service_views = views_on
    if before is not None:
        before(server)
    cluster = cluster or simple_raycluster("demo", workers=2)
    name = cluster.metadata.name
    client.create(cluster)
    for step in range(4):
        reconciler.reconcile(("default", name))
        _start_pods(server)
        if step == 0 and between is not None:
            between(server)
    rc = client.get(RayCluster, "default", name)
    assert rc.status.state == "ready"
    status = {
        "endpoints": rc.status.endpoints,
        "serviceName": rc.status.head.service_name,
        "serviceIP": rc.status.head.service_ip,
        "podIP": rc.status.head.pod_ip,
        "conditions": sorted((c.type, c.status, c.reason, c.message)
                             for c in rc.status.conditions or []),
    }
    return status, client.service_gets


def _head_service_name(cluster_name="demo"):
    c = simple_raycluster(cluster_name)
    return names.head_service_name(C.KIND_RAYCLUSTER, c.spec, cluster_name)


def _allocate_node_ports(server):
    """What an apiserver does to a NodePort Service after it is created."""
    s = server.get("Service", "default", _head_service_name())
    s["spec"]["clusterIP"] = "10.96.0.7"
    for i, port in enumerate(s["spec"]["ports"]):
        port["nodePort"] = 30000 + i
    server.update(s)


def _foreign_service(server):
    server.create({"apiVersion": "v1", "kind": "Service",
                   "metadata": {"name": _head_service_name(),
                                "namespace": "default",
                                "labels": {"made-by": "someone-else"}},
                   "spec": {"clusterIP": "10.1.2.3",
                            "ports": [{"name": "custom", "port": 1234},
                                      {"port": 99},
                                      {"name": "np", "port": 1, "nodePort": 31111}]}})


def _odd_foreign_service(server):
    """One the view does not describe: the typed path must answer."""
    server.create({"apiVersion": "v1", "kind": "Service",
                   "metadata": {"name": _head_service_name(),
                                "namespace": "default"},
                   "spec": {"clusterIP": "10.1.2.4",
                            "ports": [{"name": "lax", "port": "1234"}]}})


@pytest.mark.parametrize("backend_cls", BACKENDS)
@pytest.mark.parametrize("case", ["default", "cluster-ip", "node-port",
                                  "headless", "foreign", "odd-foreign",
                                  "client-without-views"])
def test_status_is_the_same_with_views_on_and_off(case, backend_cls, monkeypatch):
    kwargs = {}
    expect_views_used = True
    if case == "cluster-ip":
        monkeypatch.setenv(C.ENABLE_RAY_HEAD_CLUSTER_IP_SERVICE, "true")
    elif case == "node-port":
        monkeypatch.setenv(C.ENABLE_RAY_HEAD_CLUSTER_IP_SERVICE, "true")
        cluster = simple_raycluster("demo", workers=2)
        cluster.spec.head_group_spec.service_type = "NodePort"
        kwargs = {"cluster": cluster, "between": _allocate_node_ports}
    elif case == "headless":
        monkeypatch.delenv(C.ENABLE_RAY_HEAD_CLUSTER_IP_SERVICE, raising=False)
    elif case == "foreign":
        kwargs = {"before": _foreign_service}
    elif case == "odd-foreign":
        kwargs = {"before": _odd_foreign_service}
        expect_views_used = False
    elif case == "client-without-views":
        kwargs = {"client_cls": NoViewClient}
        expect_views_used = False

    def fresh(kw):
        # a cluster object is edited by the run it is handed to
        kw = dict(kw)
        if "cluster" in kw:
            kw["cluster"] = kw["cluster"].clone()
        return kw

    on, gets_on = _published_status(True, backend_cls, **fresh(kwargs))
    off, gets_off = _published_status(False, backend_cls, **fresh(kwargs))
    assert on == off
    # the cases are what they say they are
    assert on["serviceName"] == _head_service_name()
    assert on["endpoints"]
    if case in ("default", "headless"):
        assert on["serviceIP"] == on["podIP"] == "10.244.0.1"
    elif case == "cluster-ip":
        assert on["serviceIP"] is None
    elif case == "node-port":
        assert on["serviceIP"] == "10.96.0.7"
        assert set(on["endpoints"].values()) <= {str(30000 + i) for i in range(16)}
    elif case == "foreign":
        assert on["serviceIP"] == "10.1.2.3"
        assert on["endpoints"] == {"custom": "1234", "np": "31111"}
    elif case == "odd-foreign":
        assert on["endpoints"] == {"lax": "1234"}
    # and the views are what answered
    assert gets_off > 0
    if expect_views_used:
        assert gets_on < gets_off
        # the only typed read left is the one that finds no Service yet
        assert gets_on <= 1
    else:
        assert gets_on == gets_off
