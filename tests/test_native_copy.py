"""The engine's model-tree copier (kuberay_amd/_native/tree_copy.hpp) against
copy.deepcopy: same values, same types at every node, nothing shared that
deepcopy does not share, aliasing kept, every unsupported node declined to
the fallback, and no reference or allocation leaked on any path."""
import collections
import copy
import enum
import gc
import glob
import os
import sys
import threading

import pytest
import yaml
from pydantic import BaseModel, PrivateAttr

try:
    from kuberay_amd._native import engine
except ImportError:
    pytest.skip("native engine not built", allow_module_level=True)

from kuberay_amd.common import pod as podlib
from kuberay_amd.kube import objects as k8s
from kuberay_amd.kube.client import model_for_kind
from kuberay_amd.models import RayNodeType
from kuberay_amd.testing import ControlPlane, simple_raycluster
from kuberay_amd.utils import constants as C

SAMPLES_DIR = os.path.join(os.path.dirname(__file__), "..", "deploy", "samples")
FQDN = "demo-head-svc.default.svc.cluster.local"


@pytest.fixture(autouse=True)
def _native_copy_on(monkeypatch):
    """The copier under test regardless of KUBERAY_NATIVE_COPY in the
    environment the suite runs in."""
    assert engine.copy_configure(BaseModel)
    monkeypatch.setattr(k8s, "_native_copy", engine.copy_tree)


def declines():
    return engine.copy_stats()["declines"]


def copies():
    return engine.copy_stats()["copies"]


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def _sample_models():
    out = []
    for path in sorted(glob.glob(os.path.join(SAMPLES_DIR, "*.yaml"))):
        with open(path) as f:
            for i, doc in enumerate(yaml.safe_load_all(f)):
                if doc and doc.get("kind") in ("RayCluster", "RayJob", "RayService"):
                    out.append((f"{os.path.basename(path)}#{i}",
                                model_for_kind(doc["kind"]).from_dict(doc)))
    return out


def _cluster_spec_of(obj):
    if obj.kind == "RayCluster":
        return obj.spec
    return obj.spec.ray_cluster_spec


def _as_cluster(name, obj):
    """A RayCluster carrying the sample's cluster spec (what the RayJob and
    RayService controllers create from theirs)."""
    if obj.kind == "RayCluster":
        return obj
    spec = _cluster_spec_of(obj)
    if spec is None:
        return None
    base = simple_raycluster("from-" + obj.metadata.name)
    base.spec = spec
    return base


def _sidecar():
    return k8s.Container(name="sidecar", image="busybox",
                         env=[k8s.EnvVar(name="A", value="b")],
                         volume_mounts=[k8s.VolumeMount(name="v", mount_path="/v")])


def _build_pods(cluster, sidecar=False):
    """Head pod and one worker pod per group, the way the reconciler builds
    them."""
    pods = []
    head = cluster.spec.head_group_spec
    head_port = podlib.get_head_port(head.ray_start_params)
    template = podlib.default_head_pod_template(cluster, head, "demo-head-", head_port)
    if sidecar:
        template.spec.containers.append(_sidecar())
    pods.append(podlib.build_pod(
        template, RayNodeType.HEAD, head.ray_start_params, head_port,
        podlib.is_autoscaling_enabled(cluster.spec), None, FQDN,
        ray_version=cluster.spec.ray_version))
    for group in cluster.spec.worker_group_specs:
        template = podlib.default_worker_pod_template(
            cluster, group, "demo-worker-", FQDN, head_port, replica_index=2)
        if sidecar:
            template.spec.containers.append(_sidecar())
        pods.append(podlib.build_pod(
            template, RayNodeType.WORKER, group.ray_start_params, head_port,
            podlib.is_autoscaling_enabled(cluster.spec), None, FQDN,
            ray_version=cluster.spec.ray_version))
    return pods


def _variant_clusters():
    plain = simple_raycluster("plain", workers=3, gpus_per_worker=1)
    autoscaler = simple_raycluster(
        "autoscaler", workers=2, enableInTreeAutoscaling=True,
        autoscalerOptions={"version": "v2"})
    auth = simple_raycluster("auth", workers=1, authOptions={"mode": "token"})
    burn_in = simple_raycluster("burnin", workers=1, gpus_per_worker=8)
    burn_in.spec.worker_group_specs[0].template.metadata.annotations = {
        C.GPU_BURN_IN_ANNOTATION_KEY: "true"}
    return [("plain", plain, False), ("sidecar", plain, True),
            ("autoscaler", autoscaler, False), ("auth", auth, False),
            ("burn-in", burn_in, False), ("burn-in-sidecar", burn_in, True)]


def _all_inputs():
    out = []
    for name, obj in _sample_models():
        out.append((name, obj))
        spec = _cluster_spec_of(obj)
        if spec is None:
            continue
        out.append((name + ":spec", spec))
        out.append((name + ":head-template", spec.head_group_spec.template))
        for g in spec.worker_group_specs:
            out.append((f"{name}:template:{g.group_name}", g.template))
        cluster = _as_cluster(name, obj)
        for i, pod in enumerate(_build_pods(cluster.clone())):
            out.append((f"{name}:pod{i}", pod))
    for vname, cluster, sidecar in _variant_clusters():
        for i, pod in enumerate(_build_pods(cluster.clone(), sidecar)):
            out.append((f"variant:{vname}:pod{i}", pod))
    out += [
        ("dict-tree", {"a": [1, 2.5, "x", None, True, {"b": []}], "c": {"d": {}}}),
        ("list-root", [{"k": "v"}, [1, [2, [3]]], "s"]),
        ("empty-dict", {}),
        ("empty-list", []),
        ("nested-empties", {"a": {}, "b": [], "c": [{}], "d": {"e": [[]]}}),
        ("defaulted-model", k8s.ObjectMeta()),
        ("defaulted-pod", k8s.Pod()),
        ("extras-only", k8s.ObjectMeta.from_dict(
            {"managedFields": [{"manager": "x", "nested": {"a": [1]}}],
             "selfLink": "/x"})),
        ("big-int-and-floats", {"i": 2 ** 70, "f": float("inf"), "n": -0.0}),
    ]
    return out


INPUTS = _all_inputs()


# ---------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------

def walk_pair(src, cp, path="$"):
    """Same type at every node; leaves are the very objects deepcopy shares;
    no dict, list, set or model object is in both trees."""
    assert type(src) is type(cp), path
    if isinstance(src, BaseModel):
        assert src is not cp, path
        assert src.__pydantic_private__ is None and cp.__pydantic_private__ is None, path
        assert src.__pydantic_fields_set__ == cp.__pydantic_fields_set__, path
        assert src.__pydantic_fields_set__ is not cp.__pydantic_fields_set__, path
        assert type(cp.__pydantic_fields_set__) is set, path
        walk_pair(src.__dict__, cp.__dict__, path + ".__dict__")
        walk_pair(src.__pydantic_extra__, cp.__pydantic_extra__, path + ".__extra__")
    elif type(src) is dict:
        assert src is not cp, path
        assert list(src) == list(cp), path
        for k in src:
            walk_pair(src[k], cp[k], f"{path}.{k}")
    elif type(src) is list:
        assert src is not cp, path
        assert len(src) == len(cp), path
        for i, (a, b) in enumerate(zip(src, cp)):
            walk_pair(a, b, f"{path}[{i}]")
    else:
        assert src is cp, path  # None, bool, int, float, str are shared


def container_ids(obj, out):
    if isinstance(obj, BaseModel):
        if id(obj) in out:
            return out
        out.add(id(obj))
        out.add(id(obj.__pydantic_fields_set__))
        container_ids(obj.__dict__, out)
        if obj.__pydantic_extra__ is not None:
            container_ids(obj.__pydantic_extra__, out)
    elif isinstance(obj, dict):
        if id(obj) in out:
            return out
        out.add(id(obj))
        for v in obj.values():
            container_ids(v, out)
    elif isinstance(obj, list):
        if id(obj) in out:
            return out
        out.add(id(obj))
        for v in obj:
            container_ids(v, out)
    return out


@pytest.mark.parametrize("name,src", INPUTS, ids=[n for n, _ in INPUTS])
def test_copy_equals_deepcopy(name, src):
    before_c, before_d = copies(), declines()
    got = engine.copy_tree(src)
    assert got is not None, "declined"
    assert (copies(), declines()) == (before_c + 1, before_d)
    want = copy.deepcopy(src)
    assert got == want == src
    if isinstance(src, BaseModel):
        assert got.to_dict() == src.to_dict()
        assert got.model_dump(exclude_unset=True) == src.model_dump(exclude_unset=True)
    walk_pair(src, got)
    # deepcopy's own result passes the same walk, so the walk asks for
    # nothing deepcopy does not give
    walk_pair(src, want)
    assert not (container_ids(src, set()) & container_ids(got, set()))


def test_inputs_cover_what_the_issue_lists():
    names = [n for n, _ in INPUTS]
    assert sum(":pod" in n for n in names) >= 20
    assert any(n.startswith("ray-job") for n in names)
    assert any(n.startswith("ray-service") for n in names)
    assert any(n.startswith("ray-cluster") for n in names)
    pods = {n: p for n, p in INPUTS if n.startswith("variant:")}
    assert any(c.name == "sidecar" for c in pods["variant:sidecar:pod1"].spec.containers)
    assert pods["variant:autoscaler:pod1"].spec.restart_policy == "Never"
    assert pods["variant:burn-in:pod1"].spec.containers[0].startup_probe is not None
    assert any(e.name == C.RAY_AUTH_TOKEN_ENV_VAR
               for e in pods["variant:auth:pod1"].spec.containers[0].env)


def test_clone_goes_through_the_copier():
    pod = dict(INPUTS)["variant:plain:pod1"]
    before = copies()
    cloned = pod.clone()
    assert copies() == before + 1
    assert cloned == pod and cloned is not pod
    assert k8s.deep_copy(None) is None


def test_mutating_the_copy_leaves_the_source():
    pod = dict(INPUTS)["variant:plain:pod1"].clone()
    snapshot = pod.to_dict()
    cp = pod.clone()
    cp.metadata.labels["x"] = "y"
    cp.spec.containers[0].env.append(k8s.EnvVar(name="NEW", value="1"))
    cp.spec.containers[0].resources.limits["cpu"] = "99"
    cp.spec.node_selector = {"a": "b"}
    assert pod.to_dict() == snapshot
    assert "node_selector" in cp.spec.__pydantic_fields_set__


# ---------------------------------------------------------------------------
# aliasing
# ---------------------------------------------------------------------------

def test_one_list_referenced_twice_stays_one_object():
    shared = ["a", {"b": 1}]
    src = {"x": shared, "y": {"z": shared}}
    got = engine.copy_tree(src)
    assert got == src
    assert got["x"] is got["y"]["z"] and got["x"] is not shared
    assert got["x"][1] is got["y"]["z"][1]


def test_one_model_and_one_dict_referenced_twice():
    env = k8s.EnvVar(name="A", value="1")
    limits = {"cpu": "1"}
    c = k8s.Container(name="c")
    c.env = [env, env]
    c.resources = k8s.ResourceRequirements()
    c.resources.limits = limits
    c.resources.requests = limits
    got = engine.copy_tree(c)
    want = copy.deepcopy(c)
    assert got == want
    assert got.env[0] is got.env[1] and got.env[0] is not env
    assert want.env[0] is want.env[1]
    assert got.resources.limits is got.resources.requests
    assert got.resources.limits is not limits


def test_self_containing_dict_and_list_are_reproduced():
    d = {"k": "v"}
    d["self"] = d
    got = engine.copy_tree(d)
    assert got is not d and got["self"] is got and got["k"] == "v"
    lst = [1]
    lst.append(lst)
    got = engine.copy_tree(lst)
    assert got is not lst and got[1] is got and got[0] == 1


def test_model_inside_itself_declines():
    m = k8s.ObjectMeta()
    m.labels = {"me": m}
    before = declines()
    assert engine.copy_tree(m) is None
    assert declines() == before + 1


def test_dict_in_a_model_typed_field_is_copied_as_a_dict():
    pod = k8s.Pod()
    pod.metadata = {"name": "x", "labels": {"a": "b"}}
    pod.spec.containers = [{"name": "raw"}]
    got = engine.copy_tree(pod)
    assert type(got.metadata) is dict and got.metadata == pod.metadata
    assert got.metadata is not pod.metadata
    assert got.metadata["labels"] is not pod.metadata["labels"]
    assert type(got.spec.containers[0]) is dict
    walk_pair(pod, got)


# ---------------------------------------------------------------------------
# declines
# ---------------------------------------------------------------------------

class MyStr(str):
    pass


class MyInt(int):
    pass


class MyFloat(float):
    pass


class MyDict(dict):
    pass


class MyList(list):
    pass


class Color(enum.Enum):
    RED = "red"


class StrColor(str, enum.Enum):
    RED = "red"


class WithPrivate(k8s.K8sModel):
    name: str = "p"
    _secret: int = PrivateAttr(default=7)


class OwnDeepcopy(k8s.K8sModel):
    name: str = "o"

    def __deepcopy__(self, memo=None):
        out = type(self)(name=self.name + "-copied")
        return out


def _nested_lists(depth):
    root = cur = []
    for _ in range(depth):
        nxt = []
        cur.append(nxt)
        cur = nxt
    return root


def _nested_models(depth):
    root = cur = k8s.ObjectMeta()
    for _ in range(depth):
        nxt = k8s.ObjectMeta()
        cur.labels = {"next": nxt}
        cur = nxt
    return root


def _fields_set_subclass():
    m = k8s.ObjectMeta(name="x")
    object.__setattr__(m, "__pydantic_fields_set__", frozenset({"name"}))
    return m


def _extra_not_a_dict():
    m = k8s.ObjectMeta(name="x")
    object.__setattr__(m, "__pydantic_extra__", collections.OrderedDict(a=1))
    return m


DECLINED_VALUES = [
    ("tuple", ("a", "b")),
    ("empty-tuple", ()),
    ("set", {"a"}),
    ("frozenset", frozenset({"a"})),
    ("bytes", b"x"),
    ("str-subclass", MyStr("s")),
    ("int-subclass", MyInt(3)),
    ("float-subclass", MyFloat(1.5)),
    ("dict-subclass", MyDict(a=1)),
    ("ordered-dict", collections.OrderedDict(a=1)),
    ("list-subclass", MyList([1])),
    ("enum", Color.RED),
    ("str-enum", StrColor.RED),
    ("int-key", {1: "a"}),
    ("tuple-key", {("a",): "a"}),
    ("str-subclass-key", {MyStr("k"): "a"}),
    ("private-attrs", WithPrivate()),
    ("own-deepcopy", OwnDeepcopy()),
    ("too-deep-lists", _nested_lists(200)),
    ("too-deep-models", _nested_models(60)),
    ("fields-set-not-a-set", _fields_set_subclass()),
    ("extra-not-a-dict", _extra_not_a_dict()),
    ("complex", 1 + 2j),
]


@pytest.mark.parametrize("where", ["root", "dict-value", "list-item",
                                   "model-field", "model-extra"])
@pytest.mark.parametrize("name,value", DECLINED_VALUES,
                         ids=[n for n, _ in DECLINED_VALUES])
def test_declined_trees_fall_back_to_deepcopy(name, value, where):
    if where == "root":
        src = value
    elif where == "dict-value":
        src = {"ok": [1, 2], "bad": value}
    elif where == "list-item":
        src = [{"ok": 1}, value]
    elif where == "model-field":
        src = k8s.Pod()
        src.metadata.labels = {"ok": "1"}
        src.spec.affinity = value
    else:
        src = k8s.Pod()
        src.spec.__pydantic_extra__["somethingElse"] = value
    before_d, before_c = declines(), copies()
    assert engine.copy_tree(src) is None
    assert (declines(), copies()) == (before_d + 1, before_c)
    # the helper and clone() give what deepcopy gives
    want = copy.deepcopy(src)
    before_d = declines()
    got = src.clone() if isinstance(src, k8s.K8sModel) else k8s.deep_copy(src)
    assert declines() == before_d + 1
    assert type(got) is type(want)
    assert got == want
    if name == "own-deepcopy" and where == "root":
        assert got.name == "o-copied"


def test_depth_limit_is_a_decline_not_a_crash():
    ok = _nested_lists(100)
    assert engine.copy_tree(ok) == ok
    assert engine.copy_tree(_nested_lists(5000)) is None


def test_disabled_copier_declines_everything():
    try:
        assert engine.copy_configure(None) is False
        before = declines()
        assert engine.copy_tree({"a": 1}) is None
        assert declines() == before + 1

        class NoSlots:
            pass
        assert engine.copy_configure(NoSlots) is False
        assert engine.copy_configure("not a type") is False
        assert engine.copy_tree(k8s.Pod()) is None
    finally:
        assert engine.copy_configure(BaseModel) is True
    assert engine.copy_tree({"a": 1}) == {"a": 1}


def test_switch_forces_the_fallback(monkeypatch):
    monkeypatch.setattr(k8s, "_native_copy", None)
    pod = dict(INPUTS)["variant:plain:pod1"]
    before = engine.copy_stats()
    cloned = pod.clone()
    assert engine.copy_stats() == before
    assert cloned == pod and cloned is not pod


def test_switch_is_read_from_the_environment_at_import():
    import subprocess
    code = ("from kuberay_amd.kube import objects as o; "
            "print(o._native_copy is None)")
    for value, expect in (("0", "True"), ("1", "False")):
        env = dict(os.environ, KUBERAY_NATIVE_COPY=value)
        out = subprocess.run([sys.executable, "-c", code], env=env, text=True,
                             capture_output=True, check=True,
                             cwd=os.path.join(os.path.dirname(__file__), ".."))
        assert out.stdout.strip() == expect


# ---------------------------------------------------------------------------
# references and allocations
# ---------------------------------------------------------------------------

def test_declined_calls_leave_refcounts_unchanged():
    bad = ("sentinel-tuple",)
    leaf = "".join(["uniq", "ue-", "leaf"])
    inner = {"leaf": leaf}
    env = k8s.EnvVar(name="A", value=leaf)
    pod = k8s.Pod()
    pod.metadata.labels = {"l": leaf}
    pod.spec.containers = [k8s.Container(name="c", env=[env])]
    # the bad node comes last, so everything before it has been copied when
    # the call declines
    pod.spec.affinity = {"inner": inner, "list": [inner, env], "bad": bad}
    tracked = [bad, leaf, inner, env, pod, pod.spec, pod.metadata,
               pod.metadata.labels, pod.spec.containers, type(pod), type(env)]
    gc.collect()
    before = [sys.getrefcount(o) for o in tracked]
    for _ in range(1000):
        assert engine.copy_tree(pod) is None
    gc.collect()
    assert [sys.getrefcount(o) for o in tracked] == before


def test_leaf_refcount_follows_the_live_copies():
    leaf = "".join(["another-", "unique-", "leaf"])
    pod = dict(INPUTS)["variant:plain:pod1"].clone()
    pod.metadata.labels["leaf"] = leaf
    gc.collect()
    base = sys.getrefcount(leaf)
    held = [engine.copy_tree(pod) for _ in range(7)]
    assert sys.getrefcount(leaf) == base + 7
    held.pop()
    assert sys.getrefcount(leaf) == base + 6
    del held
    gc.collect()
    assert sys.getrefcount(leaf) == base
    # type objects are referenced by their instances only
    pod_type = k8s.Pod
    tp_base = sys.getrefcount(pod_type)
    held = [engine.copy_tree(pod) for _ in range(5)]
    assert sys.getrefcount(pod_type) == tp_base + 5
    del held
    gc.collect()
    assert sys.getrefcount(pod_type) == tp_base


def test_allocated_blocks_flat_over_copy_and_drop():
    pod = dict(INPUTS)["variant:burn-in-sidecar:pod1"]
    declined = {"a": [pod, ("t",)]}

    def rounds(n):
        for _ in range(n):
            engine.copy_tree(pod)
            engine.copy_tree(declined)

    rounds(200)
    gc.collect()
    before = sys.getallocatedblocks()
    rounds(10_000)
    gc.collect()
    after = sys.getallocatedblocks()
    # a built pod is a few hundred blocks; one leaked per round would be 10 000
    assert abs(after - before) < 100, (before, after)


def test_four_threads_copy_one_shared_source():
    pod = dict(INPUTS)["variant:sidecar:pod1"]
    want = pod.to_dict()
    errors = []

    def work():
        try:
            for i in range(2000):
                got = engine.copy_tree(pod)
                if got is None or got != pod:
                    errors.append("unequal copy")
                    return
                if i % 250 == 0 and got.to_dict() != want:
                    errors.append("to_dict differs")
                    return
        except Exception as e:  # pragma: no cover
            errors.append(repr(e))

    threads = [threading.Thread(target=work) for _ in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
    assert pod.to_dict() == want


# ---------------------------------------------------------------------------
# the bench's shape
# ---------------------------------------------------------------------------

def test_bench_shaped_run_has_no_declines():
    before_d, before_c = declines(), copies()
    cp = ControlPlane(kubelet_delay=0.0, poll_seconds=0.05)
    cp.start()
    try:
        names = [f"bench-{i}" for i in range(5)]
        for n in names:
            cp.client.create(simple_raycluster(n, workers=3, gpus_per_worker=1))
        for n in names:
            assert cp.wait_cluster_state("default", n, "ready", timeout=30)
        from kuberay_amd.models import RayCluster
        for n in names:
            cp.client.delete(RayCluster, "default", n)
        assert cp.wait_for(lambda: cp.server.count("Pod") == 0, timeout=30)
    finally:
        cp.stop()
    assert declines() == before_d
    # per cluster at least: the spec hash, two clones each for the head pod
    # and the first worker pod, one per further replica
    assert copies() - before_c >= 5 * (1 + 2 + 2 + 2)
