"""In-memory Kubernetes API server (the envtest analog, plus a GC).

The reference tests its reconcilers against a real kube-apiserver spun up by
controller-runtime's envtest (ray-operator/controllers/ray/suite_test.go:77-120)
with NO kubelet — pods never actually run. This module provides the same
seam natively: a thread-safe object store with resourceVersion semantics,
optimistic-concurrency conflicts, finalizer-aware deletion, ownerReference
garbage collection and label-selector lists + watches.

Storage is pluggable (the semantic layer is backend-agnostic):

* ``PyBackend`` — plain python dict trees (always available),
* ``NativeBackend`` (kuberay_amd/kube/native.py) — the C++ engine: objects
  live as compact JSON blobs in C++ with label/owner indexes and
  precomputed pod *views*, so the 500-cluster / 2000-pod cache holds no
  Python object trees at all (RSS) and the reconcile hot loop reads tiny
  projections instead of materializing pods.

``InMemoryApiServer()`` picks the native backend automatically when the
extension is built.
"""
from __future__ import annotations

import dataclasses
import threading
import time
import uuid
from collections import defaultdict, deque
from typing import Any, Dict, Iterable, List, Optional, Tuple

Key = Tuple[str, str, str]  # (kind, namespace, name)


def jsoncopy(obj):
    """Deep copy for JSON-shaped trees (dict/list/scalars only) — ~4x faster
    than copy.deepcopy, which pays for memoization and type dispatch these
    trees never need."""
    t = type(obj)
    if t is dict:
        return {k: jsoncopy(v) for k, v in obj.items()}
    if t is list:
        return [jsoncopy(v) for v in obj]
    return obj


class ApiError(Exception):
    def __init__(self, code: int, message: str):
        super().__init__(f"{code}: {message}")
        self.code = code
        self.message = message


class NotFoundError(ApiError):
    def __init__(self, message: str = "not found"):
        super().__init__(404, message)


class ConflictError(ApiError):
    def __init__(self, message: str = "conflict"):
        super().__init__(409, message)


class AlreadyExistsError(ApiError):
    def __init__(self, message: str = "already exists"):
        super().__init__(409, message)


class GoneError(ApiError):
    """410 — watch resourceVersion too old; re-list and re-watch."""

    def __init__(self, message: str = "resource version too old"):
        super().__init__(410, message)


def now_iso() -> str:
    return time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())


def match_labels(labels: Optional[Dict[str, str]], selector: Optional[Dict[str, str]]) -> bool:
    if not selector:
        return True
    labels = labels or {}
    return all(labels.get(k) == v for k, v in selector.items())


# ---------------------------------------------------------------------------
# pod views — the reconcile hot-loop projection, precomputed at write time
# ---------------------------------------------------------------------------

@dataclasses.dataclass
class PodView:
    name: str
    namespace: str
    labels: Dict[str, str]
    phase: str = ""
    ready: bool = False
    deletion_timestamp: str = ""
    pod_ip: str = ""
    restart_policy: str = ""
    ray_container_terminated: bool = False
    creation_timestamp: str = ""


def compute_pod_view(obj: Dict[str, Any]) -> PodView:
    meta = obj.get("metadata", {})
    status = obj.get("status") or {}
    spec = obj.get("spec") or {}
    ready = any(c.get("type") == "Ready" and c.get("status") == "True"
                for c in status.get("conditions") or [])
    terminated = False
    containers = spec.get("containers") or []
    if containers:
        ray_name = containers[0].get("name")
        for cs in status.get("containerStatuses") or []:
            if cs.get("name") == ray_name and (cs.get("state") or {}).get("terminated"):
                terminated = True
    return PodView(
        name=meta.get("name", ""),
        namespace=meta.get("namespace", "default"),
        labels=dict(meta.get("labels") or {}),
        phase=status.get("phase") or "",
        ready=ready,
        deletion_timestamp=meta.get("deletionTimestamp") or "",
        pod_ip=status.get("podIP") or "",
        restart_policy=spec.get("restartPolicy") or "",
        ray_container_terminated=terminated,
        creation_timestamp=meta.get("creationTimestamp") or "",
    )


# ---------------------------------------------------------------------------
# service views — what the RayCluster reconciler reads from the head Service
# ---------------------------------------------------------------------------

@dataclasses.dataclass
class ServiceView:
    name: str
    namespace: str
    cluster_ip: str = ""  # "" when the Service has none
    # (name or "", port or None, nodePort or None) per port
    ports: List[Tuple[str, Optional[int], Optional[int]]] = dataclasses.field(
        default_factory=list)


_INT64 = 1 << 63


def _view_port_number(value):
    """None or an exact int64 passes; anything else (bool, str, float,
    subclass) has no place in a view."""
    if value is None:
        return True
    return type(value) is int and -_INT64 <= value < _INT64


def compute_service_view(obj: Dict[str, Any]) -> Optional[ServiceView]:
    """The view of a stored Service, or None when the object has a shape the
    view does not describe exactly; readers then take the typed path, so a
    view is never wrong. The engine computes the same from the tree it
    encodes (extract_service_view in _native/engine.cpp)."""
    meta = obj.get("metadata", {})
    if type(meta) is not dict:
        return None
    name = meta.get("name", "")
    namespace = meta.get("namespace", "default")
    if type(name) is not str or type(namespace) is not str:
        return None
    view = ServiceView(name=name, namespace=namespace)
    if "spec" not in obj:
        return view
    spec = obj["spec"]
    if type(spec) is not dict:
        return None
    ip = spec.get("clusterIP")
    if ip is not None:
        if type(ip) is not str or not ip:
            return None  # "" and "no clusterIP" differ
        view.cluster_ip = ip
    ports = spec.get("ports")
    if ports is None:
        return view
    if type(ports) is not list:
        return None
    for port in ports:
        if type(port) is not dict:
            return None
        pname = port.get("name")
        if pname is None:
            pname = ""
        number, node_port = port.get("port"), port.get("nodePort")
        if (type(pname) is not str or not _view_port_number(number)
                or not _view_port_number(node_port)):
            return None
        view.ports.append((pname, number, node_port))
    return view


# ---------------------------------------------------------------------------
# storage backends
# ---------------------------------------------------------------------------

class PyBackend:
    """Plain python dict storage. Copy-on-put + copy-on-fetch keeps stored
    trees private."""

    name = "python"

    def __init__(self) -> None:
        self._objects: Dict[Key, Dict[str, Any]] = {}
        self._views: Dict[Key, PodView] = {}
        self._service_views: Dict[Key, ServiceView] = {}
        self._label_index: Dict[Tuple[str, str, str], set] = defaultdict(set)
        self._kind_index: Dict[str, set] = defaultdict(set)
        self._owner_index: Dict[str, set] = defaultdict(set)

    def put(self, key: Key, obj: Dict[str, Any]) -> None:
        old = self._objects.get(key)
        if old is not None:
            self._index_remove(key, old)
        stored = jsoncopy(obj)
        self._objects[key] = stored
        self._index_add(key, stored)
        if key[0] == "Pod":
            self._views[key] = compute_pod_view(stored)
        elif key[0] == "Service":
            view = compute_service_view(stored)
            if view is not None:
                self._service_views[key] = view
            else:
                self._service_views.pop(key, None)

    def fetch(self, key: Key) -> Optional[Dict[str, Any]]:
        obj = self._objects.get(key)
        return jsoncopy(obj) if obj is not None else None

    def kinds(self):
        return [k for k, keys in self._kind_index.items() if keys]

    def rv(self, key: Key) -> Optional[str]:
        obj = self._objects.get(key)
        return obj["metadata"].get("resourceVersion") if obj is not None else None

    def contains(self, key: Key) -> bool:
        return key in self._objects

    def remove(self, key: Key) -> Optional[Dict[str, Any]]:
        obj = self._objects.pop(key, None)
        if obj is not None:
            self._index_remove(key, obj)
            self._views.pop(key, None)
            self._service_views.pop(key, None)
        return obj

    def service_view(self, key: Key) -> Optional[ServiceView]:
        return self._service_views.get(key)

    def _select_keys(self, kind: str, namespace: Optional[str],
                     selector: Optional[Dict[str, str]]) -> List[Key]:
        if selector:
            candidate_sets = [self._label_index.get((kind, k, v), set())
                              for k, v in selector.items()]
            keys: Iterable[Key] = (set.intersection(*candidate_sets)
                                   if candidate_sets else set())
        else:
            keys = self._kind_index.get(kind, set())
        return [k for k in keys if namespace is None or k[1] == namespace]

    def list(self, kind: str, namespace: Optional[str],
             selector: Optional[Dict[str, str]]) -> List[Dict[str, Any]]:
        out = [jsoncopy(self._objects[k])
               for k in self._select_keys(kind, namespace, selector)
               if k in self._objects]
        out.sort(key=lambda o: (o["metadata"]["namespace"], o["metadata"]["name"]))
        return out

    def list_views(self, namespace: Optional[str],
                   selector: Optional[Dict[str, str]]) -> List[PodView]:
        out = [self._views[k]
               for k in self._select_keys("Pod", namespace, selector)
               if k in self._views]
        out.sort(key=lambda v: (v.namespace, v.name))
        return out

    def dependents(self, uid: str) -> List[Key]:
        return list(self._owner_index.get(uid, ()))

    def drop_owner(self, uid: str) -> None:
        self._owner_index.pop(uid, None)

    def count(self, kind: str) -> int:
        return len(self._kind_index.get(kind, ()))

    # -- index internals ----------------------------------------------
    def _index_add(self, key: Key, obj: Dict[str, Any]) -> None:
        self._kind_index[key[0]].add(key)
        meta = obj.get("metadata", {})
        for lk, lv in (meta.get("labels") or {}).items():
            self._label_index[(key[0], lk, lv)].add(key)
        for ref in meta.get("ownerReferences") or []:
            uid = ref.get("uid")
            if uid:
                self._owner_index[uid].add(key)

    def _index_remove(self, key: Key, obj: Dict[str, Any]) -> None:
        self._kind_index[key[0]].discard(key)
        meta = obj.get("metadata", {})
        for lk, lv in (meta.get("labels") or {}).items():
            self._label_index[(key[0], lk, lv)].discard(key)
        for ref in meta.get("ownerReferences") or []:
            uid = ref.get("uid")
            if uid:
                self._owner_index[uid].discard(key)


def default_backend():
    """Native C++ backend when built, python otherwise."""
    try:
        from .native import NativeBackend
        return NativeBackend()
    except ImportError:
        return PyBackend()


# ---------------------------------------------------------------------------
# semantic layer
# ---------------------------------------------------------------------------

class InMemoryApiServer:
    """Thread-safe object store with Kubernetes verb semantics."""

    # events retained for resourceVersion-based watch resumption; a client
    # asking for an rv older than this window gets 410 Gone (real-apiserver
    # etcd-compaction semantics)
    EVENT_HISTORY_LIMIT = 1024

    def __init__(self, backend=None) -> None:
        self._lock = threading.RLock()
        self._backend = backend if backend is not None else default_backend()
        self._rv = 0
        self._watchers: List["Watcher"] = []
        self._event_history: deque = deque(maxlen=self.EVENT_HISTORY_LIMIT)
        # lowest rv from which a watch can replay with proven completeness;
        # raised on snapshot restore (pre-restart events are gone — clients
        # below it must get 410 and re-list, never a silent gap)
        self._history_base: int = 0
        # optional backend fast paths (the native engine has them): the
        # backend records the watch history itself, in the same call as the
        # write and from the bytes it stores anyway, splices status writes
        # and answers delete's questions without parsing. Any backend
        # without them gets the plain put/fetch/remove protocol and the
        # python history above.
        self._fast = all(hasattr(self._backend, n) for n in (
            "put_status", "peek", "history_since", "history_reset"))
        if self._fast:
            self._backend.history_reset(0, self.EVENT_HISTORY_LIMIT)

    @property
    def backend_name(self) -> str:
        return self._backend.name

    # -- internals -----------------------------------------------------
    def _next_rv(self) -> str:
        self._rv += 1
        return str(self._rv)

    def _put(self, key: Key, obj: Dict[str, Any], event_type: str,
             status_only: bool = False) -> None:
        """Backend write (lock held). On the fast path the history entry for
        ``event_type`` is recorded by the same call."""
        if not self._fast:
            self._backend.put(key, obj)
        elif status_only:
            self._backend.put_status(key, obj, event_type)
        else:
            self._backend.put(key, obj, event_type)

    def _notify(self, event_type: str, obj: Dict[str, Any]) -> None:
        if not self._fast:
            try:
                rv = int(obj.get("metadata", {}).get("resourceVersion") or self._rv)
            except (TypeError, ValueError):
                rv = self._rv
            if event_type == "DELETED":
                # real apiserver: a delete is itself a new revision
                rv = self._rv
            # history entries are stored SERIALIZED: one compact string
            # instead of ~10² nested dicts per event keeps the 1024-entry
            # window at ~1 MB instead of ~11 MB resident (replay decodes on
            # demand)
            import json as _json
            self._event_history.append(
                (rv, event_type, obj.get("kind", ""),
                 _json.dumps(obj, separators=(",", ":"))))
        for w in list(self._watchers):
            w.push(event_type, obj)

    def reset_history(self, rv: int) -> None:
        """Snapshot restore: continue from revision ``rv`` with an empty
        watch history. Events before the restore point are unreplayable, so
        watchers resuming below it must get 410 and re-list."""
        with self._lock:
            self._rv = rv
            self._history_base = rv
            self._event_history.clear()
            if self._fast:
                self._backend.history_reset(rv, self.EVENT_HISTORY_LIMIT)

    @property
    def current_rv(self) -> int:
        with self._lock:
            return self._rv

    def events_since(self, rv: int, kinds: Optional[set] = None):
        """Events with resourceVersion > rv, oldest first.

        Returns None when the requested rv predates the retained history —
        the watch must be answered with 410 Gone and the client re-lists
        (kube-apiserver 'too old resource version' semantics).
        """
        if self._fast:
            # the engine keeps the ring; blobs are decoded on demand and a
            # DELETED entry gets the delete's own rv put back in
            return self._backend.history_since(rv, kinds)
        import json as _json
        with self._lock:
            hist = self._event_history
            if rv < self._history_base:
                return None
            if len(hist) == hist.maxlen and hist[0][0] > rv + 1:
                return None
            return [(etype, _json.loads(payload))
                    for (erv, etype, kind, payload) in hist
                    if erv > rv and (kinds is None or kind in kinds)]

    @staticmethod
    def _key_of(obj: Dict[str, Any]) -> Key:
        meta = obj.get("metadata", {})
        return (obj.get("kind", ""), meta.get("namespace", "default"),
                meta.get("name", ""))

    # -- verbs ---------------------------------------------------------
    def create(self, obj: Dict[str, Any], *, assume_owned: bool = False) -> Dict[str, Any]:
        if not assume_owned:
            obj = jsoncopy(obj)
        meta = obj.setdefault("metadata", {})
        meta.setdefault("namespace", "default")
        if not meta.get("name"):
            gen = meta.get("generateName")
            if not gen:
                raise ApiError(422, "name or generateName required")
            meta["name"] = gen + uuid.uuid4().hex[:5]
        with self._lock:
            key = self._key_of(obj)
            if self._backend.contains(key):
                raise AlreadyExistsError(f"{key} already exists")
            meta["uid"] = str(uuid.uuid4())
            meta["resourceVersion"] = self._next_rv()
            meta["generation"] = 1
            meta["creationTimestamp"] = now_iso()
            self._put(key, obj, "ADDED")
        self._notify("ADDED", obj)
        return obj

    def get(self, kind: str, namespace: str, name: str) -> Dict[str, Any]:
        with self._lock:
            obj = self._backend.fetch((kind, namespace, name))
        if obj is None:
            raise NotFoundError(f"{kind} {namespace}/{name} not found")
        return obj

    def try_get(self, kind: str, namespace: str, name: str) -> Optional[Dict[str, Any]]:
        with self._lock:
            return self._backend.fetch((kind, namespace, name))

    def list(self, kind: str, namespace: Optional[str] = None,
             label_selector: Optional[Dict[str, str]] = None) -> List[Dict[str, Any]]:
        with self._lock:
            return self._backend.list(kind, namespace, label_selector)

    def kinds(self):
        """Kinds with at least one stored object (dynamic-routing support
        in the HTTP facade)."""
        with self._lock:
            fn = getattr(self._backend, "kinds", None)
            return fn() if fn else []

    def list_pod_views(self, namespace: Optional[str] = None,
                       label_selector: Optional[Dict[str, str]] = None) -> List[PodView]:
        """Reconcile-hot-loop projection (no pod materialization)."""
        with self._lock:
            return self._backend.list_views(namespace, label_selector)

    def service_view(self, namespace: str, name: str) -> Optional[ServiceView]:
        """The stored Service's view, or None when there is no such Service,
        it has no view, or the backend keeps none: callers then read the
        object itself."""
        fn = getattr(self._backend, "service_view", None)
        if fn is None:
            return None
        with self._lock:
            return fn(("Service", namespace, name))

    def update(self, obj: Dict[str, Any], *, subresource: Optional[str] = None,
               assume_owned: bool = False) -> Dict[str, Any]:
        if not assume_owned:
            obj = jsoncopy(obj)
        key = self._key_of(obj)
        with self._lock:
            current = self._backend.fetch(key)
            if current is None:
                raise NotFoundError(f"{key} not found")
            new_obj, finalizers_gone = self._apply_update(
                key, obj, current, subresource)
        self._notify("MODIFIED", new_obj)
        if finalizers_gone:
            self._finalize_delete(key)
        return new_obj

    def _apply_update(self, key: Key, obj: Dict[str, Any],
                      current: Dict[str, Any], subresource: Optional[str]):
        """The update rules, given the stored object already fetched (lock
        held; both trees are the caller's to edit). Writes the result and
        returns ``(stored object, finalizers gone while deleting)``; the
        caller notifies and finishes the delete outside the lock."""
        meta = obj.setdefault("metadata", {})
        rv = meta.get("resourceVersion")
        cur_meta = current["metadata"]
        if rv is not None and rv != cur_meta["resourceVersion"]:
            raise ConflictError(
                f"{key}: resourceVersion mismatch {rv} != {cur_meta['resourceVersion']}")
        if subresource == "status":
            # the status subresource takes everything but status from the
            # stored object
            new_obj = current
            new_obj["status"] = obj.get("status", {})
        else:
            new_obj = obj
            if new_obj.get("spec") != current.get("spec"):
                new_obj["metadata"]["generation"] = cur_meta.get("generation", 1) + 1
            else:
                new_obj["metadata"]["generation"] = cur_meta.get("generation", 1)
            new_obj["status"] = current.get("status", {})
        new_obj["metadata"]["uid"] = cur_meta["uid"]
        new_obj["metadata"]["creationTimestamp"] = cur_meta["creationTimestamp"]
        if cur_meta.get("deletionTimestamp"):
            new_obj["metadata"]["deletionTimestamp"] = cur_meta["deletionTimestamp"]
        new_obj["metadata"]["resourceVersion"] = self._next_rv()
        self._put(key, new_obj, "MODIFIED",
                  status_only=subresource == "status")
        finalizers_gone = (
            cur_meta.get("deletionTimestamp")
            and not new_obj["metadata"].get("finalizers"))
        return new_obj, finalizers_gone

    def patch_merge(self, kind: str, namespace: str, name: str,
                    patch: Dict[str, Any], *, subresource: Optional[str] = None,
                    ) -> Dict[str, Any]:
        """Strategic-merge-ish patch (recursive dict merge; lists replaced).
        One fetch, one write, one lock hold."""
        key = (kind, namespace, name)

        def merge(dst, src):
            for k, v in src.items():
                if isinstance(v, dict):
                    # RFC 7386: patch objects merge into the existing
                    # value or {} — nested nulls delete, never
                    # materialize (keeps merge patch idempotent)
                    node = dst.get(k)
                    if not isinstance(node, dict):
                        node = dst[k] = {}
                    merge(node, v)
                elif v is None:
                    dst.pop(k, None)
                else:
                    dst[k] = jsoncopy(v)

        with self._lock:
            current = self._backend.fetch(key)
            if current is None:
                raise NotFoundError(f"{kind} {namespace}/{name} not found")
            if subresource == "status":
                # only the status is taken from the patched tree
                merged = current
                merge(merged.setdefault("status", {}),
                      patch.get("status", patch))
            else:
                # the update rules compare the patched tree with the stored
                # one, so the patch goes onto a copy of the one parsed tree
                merged = jsoncopy(current)
                if subresource is not None:
                    merged.setdefault("status", {})
                merge(merged, patch)
            if self._key_of(merged) != key:
                # the patch renamed the object: update() addresses whatever
                # the patched tree names
                return self.update(merged, subresource=subresource,
                                   assume_owned=True)
            new_obj, finalizers_gone = self._apply_update(
                key, merged, current, subresource)
        self._notify("MODIFIED", new_obj)
        if finalizers_gone:
            self._finalize_delete(key)
        return new_obj

    def mutate_status(self, kind: str, namespace: str, name: str,
                      fn) -> Optional[Dict[str, Any]]:
        """Single-fetch status mutation: ``fn(obj)`` edits ``obj['status']``
        in place (or returns False to skip the write). One backend fetch and
        parse, one write, one lock hold — the sim kubelet's pod-start
        transition is hot enough at 2000-pod bursts for anything more to
        show up in profiles. ``fn`` runs under the store lock and must edit
        nothing but the status. Returns the stored object, or None when
        skipped/missing."""
        key = (kind, namespace, name)
        with self._lock:
            obj = self._backend.fetch(key)
            if obj is None:
                return None
            if fn(obj) is False:
                return None
            new_obj, finalizers_gone = self._apply_update(
                key, obj, obj, "status")
        self._notify("MODIFIED", new_obj)
        if finalizers_gone:
            self._finalize_delete(key)
        return new_obj

    def delete(self, kind: str, namespace: str, name: str) -> None:
        key = (kind, namespace, name)
        with self._lock:
            if self._fast:
                # decided from the fields the engine keeps beside the
                # object; nothing is parsed unless the delete is blocked
                peeked = self._backend.peek(key)
                if peeked is None:
                    raise NotFoundError(f"{kind} {namespace}/{name} not found")
                _, _, has_finalizers, deletion_ts = peeked
                if has_finalizers and deletion_ts:
                    return
                current = self._backend.fetch(key) if has_finalizers else None
            else:
                current = self._backend.fetch(key)
                if current is None:
                    raise NotFoundError(f"{kind} {namespace}/{name} not found")
                if not current["metadata"].get("finalizers"):
                    current = None
                elif current["metadata"].get("deletionTimestamp"):
                    return
            if current is not None:
                current["metadata"]["deletionTimestamp"] = now_iso()
                current["metadata"]["resourceVersion"] = self._next_rv()
                self._put(key, current, "MODIFIED")
        if current is not None:
            self._notify("MODIFIED", current)
            return
        self._finalize_delete(key)

    def _finalize_delete(self, key: Key) -> None:
        with self._lock:
            # a delete is its own revision (real-apiserver semantics):
            # without a fresh rv, a watcher resuming from the object's last
            # rv would treat the DELETED event as already-seen and miss it
            if self._fast:
                # the engine records the DELETED entry from the sections it
                # already holds; this parse is for the watchers
                current = self._backend.remove(key, self._rv + 1)
            else:
                current = self._backend.remove(key)
            if current is None:
                return
            current["metadata"]["resourceVersion"] = self._next_rv()
            uid = current["metadata"]["uid"]
            dependents = self._backend.dependents(uid)
            self._backend.drop_owner(uid)
        self._notify("DELETED", current)
        for dep in dependents:
            try:
                self.delete(*dep)
            except NotFoundError:
                pass

    # -- watches -------------------------------------------------------
    def watch(self, kinds: Optional[Iterable[str]] = None) -> "Watcher":
        w = Watcher(self, set(kinds) if kinds else None)
        with self._lock:
            self._watchers.append(w)
        return w

    def stop_watch(self, w: "Watcher") -> None:
        with self._lock:
            if w in self._watchers:
                self._watchers.remove(w)

    # -- introspection -------------------------------------------------
    def count(self, kind: str) -> int:
        with self._lock:
            return self._backend.count(kind)

    def contains(self, kind: str, namespace: str, name: str) -> bool:
        with self._lock:
            return self._backend.contains((kind, namespace, name))


class Watcher:
    """A watch stream: buffered (event_type, object) pairs."""

    def __init__(self, server: InMemoryApiServer, kinds: Optional[set]):
        self._server = server
        self._kinds = kinds
        self._cond = threading.Condition()
        self._events: deque = deque()
        self._stopped = False

    def push(self, event_type: str, obj: Dict[str, Any]) -> None:
        if self._kinds is not None and obj.get("kind") not in self._kinds:
            return
        with self._cond:
            if self._stopped:
                return
            self._events.append((event_type, obj))
            self._cond.notify_all()

    def next(self, timeout: Optional[float] = None) -> Optional[Tuple[str, Dict[str, Any]]]:
        with self._cond:
            if not self._events:
                self._cond.wait(timeout)
            if self._events:
                return self._events.popleft()
            return None

    def drain(self) -> List[Tuple[str, Dict[str, Any]]]:
        with self._cond:
            events, self._events = list(self._events), deque()
            return events

    def stop(self) -> None:
        with self._cond:
            self._stopped = True
            self._cond.notify_all()
        self._server.stop_watch(self)
