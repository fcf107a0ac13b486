"""NativeBackend — the storage Backend over the C++ engine
(kuberay_amd/_native/engine.cpp + store_core.hpp).

The engine owns the encoding: a write hands it the dict tree and it encodes,
indexes, computes the pod view and records the watch-history entry in one
call; a status write re-encodes metadata + status only. Objects live in the
C++ heap as shared JSON sections; a read has the engine build the dict tree
straight from those sections (json_decode.hpp), and gets the assembled blob
back as bytes, to json.loads here, for an object the decoder does not
reproduce; the reconcile hot loop reads precomputed pod and Service views
without touching any JSON at all.

Trees the native encoder declines (tuples, subclasses, non-str keys, big
ints, NaN/Inf, lone surrogates, very deep nesting) take the json.dumps +
put(blob) path and behave exactly as they always did.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, List, Optional, Tuple

from .._native import engine  # raises ImportError if not built
from .store import Key, PodView, ServiceView, compute_service_view

_dumps = json.dumps
_loads = json.loads


def _view_of(obj: Dict[str, Any]):
    status = obj.get("status") or {}
    spec = obj.get("spec") or {}
    meta = obj.get("metadata", {})
    v = engine.PodViewData()
    v.name = meta.get("name", "")
    v.ns = meta.get("namespace", "default")
    v.phase = status.get("phase") or ""
    v.deletion_ts = meta.get("deletionTimestamp") or ""
    v.pod_ip = status.get("podIP") or ""
    v.restart_policy = spec.get("restartPolicy") or ""
    v.creation_ts = meta.get("creationTimestamp") or ""
    v.ready = any(c.get("type") == "Ready" and c.get("status") == "True"
                  for c in status.get("conditions") or [])
    v.terminated = False
    containers = spec.get("containers") or []
    if containers:
        ray_name = containers[0].get("name")
        for cs in status.get("containerStatuses") or []:
            if cs.get("name") == ray_name and (cs.get("state") or {}).get("terminated"):
                v.terminated = True
                break
    return v


class NativeBackend:
    name = "native-cpp"

    # Measurement switches: with either off, that write takes the slower
    # path it replaced (json.dumps + blob put / full re-encode), so the gain
    # of each part can be told apart. Results are the same either way.
    native_encode = os.environ.get("KUBERAY_STORE_NATIVE_ENCODE", "1") != "0"
    status_splice = os.environ.get("KUBERAY_STORE_STATUS_SPLICE", "1") != "0"
    # Reads: with it on, the engine builds the dict tree straight from the
    # stored sections (json_decode.hpp); off, it assembles a blob for
    # json.loads as before. An object the decoder does not reproduce comes
    # back as that blob (bytes) either way and is parsed here.
    native_decode = os.environ.get("KUBERAY_STORE_NATIVE_DECODE", "1") != "0"

    def __init__(self, history_limit: int = 1024) -> None:
        self._store = engine.NativeStore(history_limit)
        # kind -> live-object count; NativeStore has no kind enumeration,
        # and the HTTP facade needs one for dynamic (CRD) path routing
        self._kind_counts: Dict[str, int] = {}

    def put(self, key: Key, obj: Dict[str, Any],
            event_type: Optional[str] = None) -> None:
        """Store ``obj``; with ``event_type`` the watch-history entry is
        recorded in the same native call."""
        kind, ns, name = key
        is_new = (self._store.put_object(kind, ns, name, obj, event_type)
                  if self.native_encode else None)
        if is_new is None:
            is_new = self._put_blob(key, obj, event_type)
        if is_new:
            self._kind_counts[kind] = self._kind_counts.get(kind, 0) + 1

    def _put_blob(self, key: Key, obj: Dict[str, Any],
                  event_type: Optional[str]) -> bool:
        """The path for trees the native encoder declines: CPython's encoder
        produces the blob, python the index fields."""
        kind, ns, name = key
        meta = obj.get("metadata", {})
        labels = list((meta.get("labels") or {}).items())
        owners = [ref.get("uid") for ref in meta.get("ownerReferences") or []
                  if ref.get("uid")]
        view = _view_of(obj) if kind == "Pod" else None
        service_view = None
        if kind == "Service":
            sv = compute_service_view(obj)
            if sv is not None:
                service_view = (sv.name, sv.namespace, sv.cluster_ip, sv.ports)
        blob = _dumps(obj, separators=(",", ":"))
        uid = meta.get("uid")
        deletion_ts = meta.get("deletionTimestamp") or ""
        if not isinstance(deletion_ts, str):
            deletion_ts = "set"  # only its truth is read back (peek)
        return self._store.put(
            kind, ns, name, blob, meta.get("resourceVersion", ""), labels,
            owners, view, event_type, uid if isinstance(uid, str) else "",
            bool(meta.get("finalizers")), deletion_ts, service_view)

    def put_status(self, key: Key, obj: Dict[str, Any],
                   event_type: Optional[str] = None) -> None:
        """Status-subresource write: ``obj`` is the stored object with a new
        status and resourceVersion, so only those two sections are encoded."""
        if not self.status_splice or self._store.put_status(
                key[0], key[1], key[2], obj, event_type) is None:
            self.put(key, obj, event_type)

    def fetch(self, key: Key) -> Optional[Dict[str, Any]]:
        if self.native_decode:
            obj = self._store.fetch_tree(*key)
            return _loads(obj) if type(obj) is bytes else obj
        blob = self._store.fetch(*key)
        return _loads(blob) if blob is not None else None

    def rv(self, key: Key) -> Optional[str]:
        return self._store.rv(*key)

    def peek(self, key: Key) -> Optional[Tuple[str, str, bool, str]]:
        """(resourceVersion, uid, has finalizers, deletionTimestamp) of the
        stored object without touching its JSON; None when missing."""
        return self._store.peek(*key)

    def contains(self, key: Key) -> bool:
        return self._store.contains(*key)

    def remove(self, key: Key,
               event_rv: Optional[int] = None) -> Optional[Dict[str, Any]]:
        """Remove and return the object; with ``event_rv`` the DELETED
        history entry (carrying that rv) is recorded in the same call."""
        if self.native_decode:
            blob = self._store.remove_tree(key[0], key[1], key[2], event_rv)
        else:
            blob = self._store.remove(key[0], key[1], key[2], event_rv)
        if blob is None:
            return None
        n = self._kind_counts.get(key[0], 0) - 1
        if n > 0:
            self._kind_counts[key[0]] = n
        else:
            self._kind_counts.pop(key[0], None)
        return _loads(blob) if type(blob) is bytes else blob

    def list(self, kind: str, namespace: Optional[str],
             selector: Optional[Dict[str, str]]) -> List[Dict[str, Any]]:
        if self.native_decode:
            objs = self._store.list_trees(kind, namespace,
                                          list((selector or {}).items()))
            for i, obj in enumerate(objs):
                if type(obj) is bytes:
                    objs[i] = _loads(obj)
            return objs
        blobs = self._store.list_blobs(kind, namespace,
                                       list((selector or {}).items()))
        return [_loads(b) for b in blobs]

    def list_views(self, namespace: Optional[str],
                   selector: Optional[Dict[str, str]]) -> List[PodView]:
        rows = self._store.list_views(namespace, list((selector or {}).items()))
        return [
            PodView(name=r[0], namespace=r[1], labels=r[2], phase=r[3],
                    ready=r[4], deletion_timestamp=r[5], pod_ip=r[6],
                    restart_policy=r[7], ray_container_terminated=r[8],
                    creation_timestamp=r[9])
            for r in rows
        ]

    def service_view(self, key: Key) -> Optional[ServiceView]:
        """The view the engine computed when the Service was last written in
        full; None when missing or when that write produced no view."""
        row = self._store.service_view(key[1], key[2])
        if row is None:
            return None
        return ServiceView(name=row[0], namespace=row[1], cluster_ip=row[2],
                           ports=row[3])

    def dependents(self, uid: str) -> List[Key]:
        return [tuple(t) for t in self._store.dependents(uid)]

    def drop_owner(self, uid: str) -> None:
        self._store.drop_owner(uid)

    def count(self, kind: str) -> int:
        return self._store.count(kind)

    def total_bytes(self) -> int:
        return self._store.total_bytes()

    def kinds(self) -> List[str]:
        return list(self._kind_counts)

    # -- watch history (kept in the engine, in strict rv order) ----------
    def history_since(self, rv: int, kinds: Optional[set] = None):
        """[(event type, object)] with resourceVersion > rv, oldest first,
        decoded on demand; None when rv predates the retained window."""
        if self.native_decode:
            rows = self._store.history_since_trees(rv, kinds)
        else:
            rows = self._store.history_since(rv, kinds)
        if rows is None:
            return None
        out = []
        for etype, obj, rv_override in rows:
            if type(obj) is bytes:
                obj = _loads(obj)
            if rv_override is not None:
                # a delete is its own revision; the sections still carry
                # the object's last one
                obj["metadata"]["resourceVersion"] = str(rv_override)
            out.append((etype, obj))
        return out

    def history_reset(self, base: int, capacity: int = 0) -> None:
        self._store.history_reset(base, capacity)

    def history_rvs(self) -> List[int]:
        return self._store.history_rvs()

    def stats(self) -> Dict[str, int]:
        return self._store.stats()
