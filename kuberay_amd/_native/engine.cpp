// engine — native C++ object-store backend for the kuberay-amd control plane.
//
// The reconcile path of the operator is bound by its object cache: at the
// 500-cluster soak the cache holds ~2500 objects (2000 pods),
// and a Python dict-tree store pays deep copies + GC pressure + RSS for all
// of them. This backend keeps every object as compact JSON in C++ heap with
// label / kind / owner-uid indexes beside it, plus precomputed "pod views"
// (the 9 fields the RayCluster reconciler actually reads per pod per
// reconcile) so the hot loop never materializes a pod at all, and the same
// for the head Service (its clusterIP and ports).
//
// The engine owns the encoding too: put_object / put_status walk the Python
// dict tree once, write compact JSON straight into the sections the store
// keeps (store_core.hpp), pull the index fields and the pod view out of the
// same tree and append the watch-history entry — one call per write, no
// Python str in between. A status write re-encodes metadata + status only.
//
// Semantics live in python (kuberay_amd/kube/store.py InMemoryApiServer).
// This file is the pybind11 half: bindings, the PyObject encoder and field
// extraction. Everything that needs no Python is in store_core.hpp.
// Thread-safe: the core has its own mutex, which is never held while a
// Python object is created or destroyed.

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cmath>
#include <cstdio>
#include <optional>
#include <string>
#include <unordered_set>
#include <vector>

#define KUBERAY_JSON_WITH_PYTHON
#include "json_decode.hpp"
#include "store_core.hpp"
#include "tree_copy.hpp"

namespace py = pybind11;
using namespace kuberay_store;

namespace {

// Thrown when the fast path meets anything it does not reproduce exactly;
// the caller then takes the json.dumps + put(blob) path, which behaves (and
// fails) as it always did.
struct Decline {};

// Nesting the encoder follows before it declines (json.dumps goes on to the
// interpreter's recursion limit and reports circular structures itself).
constexpr int kMaxDepth = 128;

struct Keys {
  PyObject *metadata, *status, *spec, *labels, *ownerReferences, *uid,
      *resourceVersion, *finalizers, *deletionTimestamp, *name, *ns, *phase,
      *podIP, *restartPolicy, *creationTimestamp, *conditions, *type,
      *containers, *containerStatuses, *state, *terminated, *clusterIP, *ports,
      *port, *nodePort;
};
Keys K;

void init_keys() {
  auto mk = [](const char* s) { return PyUnicode_InternFromString(s); };
  K.metadata = mk("metadata"); K.status = mk("status"); K.spec = mk("spec");
  K.labels = mk("labels"); K.ownerReferences = mk("ownerReferences");
  K.uid = mk("uid"); K.resourceVersion = mk("resourceVersion");
  K.finalizers = mk("finalizers");
  K.deletionTimestamp = mk("deletionTimestamp");
  K.name = mk("name"); K.ns = mk("namespace"); K.phase = mk("phase");
  K.podIP = mk("podIP"); K.restartPolicy = mk("restartPolicy");
  K.creationTimestamp = mk("creationTimestamp");
  K.conditions = mk("conditions"); K.type = mk("type");
  K.containers = mk("containers");
  K.containerStatuses = mk("containerStatuses"); K.state = mk("state");
  K.terminated = mk("terminated");
  K.clusterIP = mk("clusterIP"); K.ports = mk("ports"); K.port = mk("port");
  K.nodePort = mk("nodePort");
}

// ---------------------------------------------------------------------------
// encoder: exact dict / list / str / bool / None / int64 / finite float
// ---------------------------------------------------------------------------

void encode_str(PyObject* s, std::string& out) {
  Py_ssize_t n = 0;
  const char* p = PyUnicode_AsUTF8AndSize(s, &n);
  if (p == nullptr) {  // lone surrogate
    PyErr_Clear();
    throw Decline{};
  }
  static const char* hex = "0123456789abcdef";
  out.push_back('"');
  const char* run = p;
  const char* end = p + n;
  for (const char* c = p; c < end; ++c) {
    const unsigned char ch = static_cast<unsigned char>(*c);
    if (ch >= 0x20 && ch != '"' && ch != '\\') continue;
    out.append(run, c - run);
    run = c + 1;
    switch (ch) {
      case '"': out += "\\\""; break;
      case '\\': out += "\\\\"; break;
      case '\n': out += "\\n"; break;
      case '\r': out += "\\r"; break;
      case '\t': out += "\\t"; break;
      case '\b': out += "\\b"; break;
      case '\f': out += "\\f"; break;
      default:
        out += "\\u00";
        out.push_back(hex[ch >> 4]);
        out.push_back(hex[ch & 0xf]);
    }
  }
  out.append(run, end - run);
  out.push_back('"');
}

void encode(PyObject* o, std::string& out, int depth) {
  if (PyUnicode_CheckExact(o)) {
    encode_str(o, out);
  } else if (PyDict_CheckExact(o)) {
    if (depth >= kMaxDepth) throw Decline{};
    out.push_back('{');
    Py_ssize_t pos = 0;
    PyObject *k, *v;
    bool first = true;
    while (PyDict_Next(o, &pos, &k, &v)) {
      if (!PyUnicode_CheckExact(k)) throw Decline{};
      if (!first) out.push_back(',');
      first = false;
      encode_str(k, out);
      out.push_back(':');
      encode(v, out, depth + 1);
    }
    out.push_back('}');
  } else if (PyList_CheckExact(o)) {
    if (depth >= kMaxDepth) throw Decline{};
    out.push_back('[');
    const Py_ssize_t n = PyList_GET_SIZE(o);
    for (Py_ssize_t i = 0; i < n; ++i) {
      if (i) out.push_back(',');
      encode(PyList_GET_ITEM(o, i), out, depth + 1);
    }
    out.push_back(']');
  } else if (o == Py_None) {
    out += "null";
  } else if (o == Py_True) {
    out += "true";
  } else if (o == Py_False) {
    out += "false";
  } else if (PyLong_CheckExact(o)) {
    int overflow = 0;
    const long long v = PyLong_AsLongLongAndOverflow(o, &overflow);
    if (overflow) throw Decline{};
    char buf[24];
    out.append(buf, std::snprintf(buf, sizeof buf, "%lld", v));
  } else if (PyFloat_CheckExact(o)) {
    const double d = PyFloat_AS_DOUBLE(o);
    if (!std::isfinite(d)) throw Decline{};
    char* s = PyOS_double_to_string(d, 'r', 0, Py_DTSF_ADD_DOT_0, nullptr);
    if (s == nullptr) {
      PyErr_Clear();
      throw Decline{};
    }
    out += s;
    PyMem_Free(s);
  } else {
    throw Decline{};  // tuple, subclass, anything else
  }
}

// ---------------------------------------------------------------------------
// field extraction — the python expressions of NativeBackend.put /
// compute_pod_view, on exact builtin types; anything else declines
// ---------------------------------------------------------------------------

// d.get(key) on an exact dict (borrowed, nullptr when missing)
PyObject* dget(PyObject* d, PyObject* key) {
  PyObject* v = PyDict_GetItemWithError(d, key);
  if (v == nullptr && PyErr_Occurred()) {
    PyErr_Clear();
    throw Decline{};
  }
  return v;
}

bool truthy(PyObject* o) {
  if (o == nullptr || o == Py_None) return false;
  const int t = PyObject_IsTrue(o);
  if (t < 0) {
    PyErr_Clear();
    throw Decline{};
  }
  return t != 0;
}

// `o or {}` that must then answer .get(): nullptr stands for the empty dict
PyObject* dict_or_empty(PyObject* o) {
  if (!truthy(o)) return nullptr;
  if (!PyDict_CheckExact(o)) throw Decline{};
  return o;
}

// `o or []` that is then iterated: nullptr stands for the empty list
PyObject* list_or_empty(PyObject* o) {
  if (!truthy(o)) return nullptr;
  if (!PyList_CheckExact(o)) throw Decline{};
  return o;
}

std::string to_utf8(PyObject* s) {
  if (!PyUnicode_CheckExact(s)) throw Decline{};
  Py_ssize_t n = 0;
  const char* p = PyUnicode_AsUTF8AndSize(s, &n);
  if (p == nullptr) {
    PyErr_Clear();
    throw Decline{};
  }
  return std::string(p, n);
}

// `d.get(key) or ""` bound for a std::string
std::string str_or_empty(PyObject* d, PyObject* key) {
  PyObject* v = d ? dget(d, key) : nullptr;
  if (!truthy(v)) return std::string();
  return to_utf8(v);
}

// `d.get(key, dflt)` bound for a std::string (None is a TypeError there)
std::string str_default(PyObject* d, PyObject* key, const char* dflt) {
  PyObject* v = d ? dget(d, key) : nullptr;
  if (v == nullptr) return dflt;
  return to_utf8(v);
}

bool str_equals(PyObject* o, const char* lit) {
  return o != nullptr && PyUnicode_CheckExact(o) &&
         PyUnicode_CompareWithASCIIString(o, lit) == 0;
}

// obj.get("metadata", {}): nullptr when missing; anything but a dict declines
PyObject* metadata_of(PyObject* obj) {
  PyObject* meta = dget(obj, K.metadata);
  if (meta != nullptr && !PyDict_CheckExact(meta)) throw Decline{};
  return meta;
}

void extract_peek(PyObject* meta, Peek& p) {
  p.rv = str_default(meta, K.resourceVersion, "");
  PyObject* uid = meta ? dget(meta, K.uid) : nullptr;
  p.uid = (uid && PyUnicode_CheckExact(uid)) ? to_utf8(uid) : std::string();
  p.has_finalizers = truthy(meta ? dget(meta, K.finalizers) : nullptr);
  p.deletion_ts = str_or_empty(meta, K.deletionTimestamp);
}

void extract_indexes(PyObject* meta, Fields& f) {
  if (PyObject* labels = dict_or_empty(meta ? dget(meta, K.labels) : nullptr)) {
    Py_ssize_t pos = 0;
    PyObject *k, *v;
    while (PyDict_Next(labels, &pos, &k, &v)) {
      f.labels.emplace_back(to_utf8(k), to_utf8(v));
    }
  }
  if (PyObject* refs =
          list_or_empty(meta ? dget(meta, K.ownerReferences) : nullptr)) {
    const Py_ssize_t n = PyList_GET_SIZE(refs);
    for (Py_ssize_t i = 0; i < n; ++i) {
      PyObject* ref = PyList_GET_ITEM(refs, i);
      if (!PyDict_CheckExact(ref)) throw Decline{};
      PyObject* uid = dget(ref, K.uid);
      if (truthy(uid)) f.owner_uids.push_back(to_utf8(uid));
    }
  }
}

// compute_pod_view (kube/store.py), field for field
void extract_view(PyObject* obj, PyObject* meta, PodViewData& v) {
  PyObject* status = dict_or_empty(dget(obj, K.status));
  PyObject* spec = dict_or_empty(dget(obj, K.spec));
  v.name = str_default(meta, K.name, "");
  v.ns = str_default(meta, K.ns, "default");
  v.phase = str_or_empty(status, K.phase);
  v.deletion_ts = str_or_empty(meta, K.deletionTimestamp);
  v.pod_ip = str_or_empty(status, K.podIP);
  v.restart_policy = str_or_empty(spec, K.restartPolicy);
  v.creation_ts = str_or_empty(meta, K.creationTimestamp);
  v.ready = false;
  if (PyObject* conds =
          list_or_empty(status ? dget(status, K.conditions) : nullptr)) {
    const Py_ssize_t n = PyList_GET_SIZE(conds);
    for (Py_ssize_t i = 0; i < n; ++i) {
      PyObject* c = PyList_GET_ITEM(conds, i);
      if (!PyDict_CheckExact(c)) throw Decline{};
      if (str_equals(dget(c, K.type), "Ready") &&
          str_equals(dget(c, K.status), "True")) {
        v.ready = true;
        break;
      }
    }
  }
  v.terminated = false;
  PyObject* containers = spec ? dget(spec, K.containers) : nullptr;
  if (!truthy(containers)) return;
  if (!PyList_CheckExact(containers)) throw Decline{};
  PyObject* first = PyList_GET_ITEM(containers, 0);
  if (!PyDict_CheckExact(first)) throw Decline{};
  PyObject* ray_name = dget(first, K.name);
  if (ray_name == nullptr) ray_name = Py_None;
  PyObject* cstats =
      list_or_empty(status ? dget(status, K.containerStatuses) : nullptr);
  if (cstats == nullptr) return;
  const Py_ssize_t n = PyList_GET_SIZE(cstats);
  for (Py_ssize_t i = 0; i < n; ++i) {
    PyObject* cs = PyList_GET_ITEM(cstats, i);
    if (!PyDict_CheckExact(cs)) throw Decline{};
    PyObject* name = dget(cs, K.name);
    if (name == nullptr) name = Py_None;
    const int eq = PyObject_RichCompareBool(name, ray_name, Py_EQ);
    if (eq < 0) {
      PyErr_Clear();
      throw Decline{};
    }
    if (!eq) continue;
    PyObject* state = dict_or_empty(dget(cs, K.state));
    if (state != nullptr && truthy(dget(state, K.terminated))) {
      v.terminated = true;
      break;
    }
  }
}

// compute_service_view (kube/store.py), field for field. False stands for its
// None: the object has a shape the view does not describe, it gets no view,
// and readers take the typed path for it.
bool optional_port(PyObject* d, PyObject* key, int64_t& out, bool& has) {
  PyObject* v = dget(d, key);
  has = false;
  if (v == nullptr || v == Py_None) return true;
  if (!PyLong_CheckExact(v)) return false;  // bool, str, float, subclass
  int overflow = 0;
  const long long n = PyLong_AsLongLongAndOverflow(v, &overflow);
  if (overflow) return false;
  out = n;
  has = true;
  return true;
}

bool extract_service_view(PyObject* obj, PyObject* meta, ServiceViewData& v) {
  try {
    v.name = str_default(meta, K.name, "");
    v.ns = str_default(meta, K.ns, "default");
    PyObject* spec = dget(obj, K.spec);
    if (spec == nullptr) return true;
    if (!PyDict_CheckExact(spec)) return false;
    PyObject* ip = dget(spec, K.clusterIP);
    if (ip != nullptr && ip != Py_None) {
      v.cluster_ip = to_utf8(ip);
      if (v.cluster_ip.empty()) return false;  // "" and "no clusterIP" differ
    }
    PyObject* ports = dget(spec, K.ports);
    if (ports == nullptr || ports == Py_None) return true;
    if (!PyList_CheckExact(ports)) return false;
    const Py_ssize_t n = PyList_GET_SIZE(ports);
    v.ports.reserve(n);
    for (Py_ssize_t i = 0; i < n; ++i) {
      PyObject* port = PyList_GET_ITEM(ports, i);
      if (!PyDict_CheckExact(port)) return false;
      ServicePortView pv;
      PyObject* name = dget(port, K.name);
      if (name != nullptr && name != Py_None) pv.name = to_utf8(name);
      if (!optional_port(port, K.port, pv.port, pv.has_port) ||
          !optional_port(port, K.nodePort, pv.node_port, pv.has_node_port)) {
        return false;
      }
      v.ports.push_back(std::move(pv));
    }
    return true;
  } catch (const Decline&) {
    return false;
  }
}

// (name, namespace, clusterIP, [(name, port or None, nodePort or None)])
using PortTuple =
    std::tuple<std::string, std::optional<int64_t>, std::optional<int64_t>>;
using ServiceViewTuple =
    std::tuple<std::string, std::string, std::string, std::vector<PortTuple>>;

Section make_section(const std::string& scratch) {
  return std::make_shared<const std::string>(scratch.data(), scratch.size());
}

py::bytes to_bytes(const Blob& b) {
  const size_t n = b.size();
  PyObject* out = PyBytes_FromStringAndSize(nullptr, static_cast<Py_ssize_t>(n));
  if (out == nullptr) throw py::error_already_set();
  b.write(PyBytes_AS_STRING(out));
  return py::reinterpret_steal<py::bytes>(out);
}

class NativeStore {
 public:
  explicit NativeStore(size_t history_capacity) : core_(history_capacity) {}

  // Full write of a Python object tree. Returns whether the key was new, or
  // None when the fast path declines (nothing is written then).
  py::object put_object(const std::string& kind, const std::string& ns,
                        const std::string& name, py::handle obj,
                        const std::optional<std::string>& event_type) {
    static thread_local std::string rest, meta_s, status_s;
    rest.clear(); meta_s.clear(); status_s.clear();
    Blob blob;
    Fields f;
    try {
      PyObject* o = obj.ptr();
      if (!PyDict_CheckExact(o)) throw Decline{};
      bool has_meta = false, has_status = false;
      Py_ssize_t pos = 0;
      PyObject *k, *v;
      while (PyDict_Next(o, &pos, &k, &v)) {
        if (!PyUnicode_CheckExact(k)) throw Decline{};
        if (PyUnicode_CompareWithASCIIString(k, "metadata") == 0) {
          encode(v, meta_s, 1);
          has_meta = true;
        } else if (PyUnicode_CompareWithASCIIString(k, "status") == 0) {
          encode(v, status_s, 1);
          has_status = true;
        } else {
          if (!rest.empty()) rest.push_back(',');
          encode_str(k, rest);
          rest.push_back(':');
          encode(v, rest, 1);
        }
      }
      PyObject* meta = metadata_of(o);
      Peek p;
      extract_peek(meta, p);
      f.rv = std::move(p.rv); f.uid = std::move(p.uid);
      f.deletion_ts = std::move(p.deletion_ts);
      f.has_finalizers = p.has_finalizers;
      extract_indexes(meta, f);
      if (kind == "Pod") {
        extract_view(o, meta, f.view);
        f.has_view = true;
      } else if (kind == "Service") {
        f.has_service_view = extract_service_view(o, meta, f.service_view);
      }
      blob.rest = make_section(rest);
      if (has_meta) blob.meta = make_section(meta_s);
      if (has_status) blob.status = make_section(status_s);
    } catch (const Decline&) {
      core_.note_fallback();
      return py::none();
    }
    core_.note_encode(true, rest.size() + meta_s.size() + status_s.size());
    const bool is_new = core_.put(kind, ns, name, std::move(blob), std::move(f),
                                  event_type ? event_type->c_str() : nullptr);
    return py::bool_(is_new);
  }

  // Status write: metadata + status re-encoded, everything else kept.
  // Returns True, or None when it cannot splice (missing key, blob entry,
  // or a tree the fast path declines) and the caller must do a full put.
  py::object put_status(const std::string& kind, const std::string& ns,
                        const std::string& name, py::handle obj,
                        const std::optional<std::string>& event_type) {
    static thread_local std::string meta_s, status_s;
    meta_s.clear(); status_s.clear();
    Section meta_sec, status_sec;
    Peek p;
    PodViewData view;
    const bool is_pod = kind == "Pod";
    try {
      PyObject* o = obj.ptr();
      if (!PyDict_CheckExact(o)) throw Decline{};
      PyObject* meta = metadata_of(o);
      if (meta != nullptr) {
        encode(meta, meta_s, 1);
        meta_sec = make_section(meta_s);
      }
      if (PyObject* status = dget(o, K.status)) {
        encode(status, status_s, 1);
        status_sec = make_section(status_s);
      }
      extract_peek(meta, p);
      if (is_pod) extract_view(o, meta, view);
    } catch (const Decline&) {
      return py::none();
    }
    if (!core_.put_status(kind, ns, name, std::move(meta_sec),
                          std::move(status_sec), std::move(p), is_pod,
                          std::move(view),
                          event_type ? event_type->c_str() : nullptr)) {
      return py::none();
    }
    core_.note_encode(false, meta_s.size() + status_s.size());
    return py::bool_(true);
  }

  // Write of a ready-made blob (the path for trees the encoder declines).
  bool put(const std::string& kind, const std::string& ns,
           const std::string& name, const std::string& blob,
           const std::string& rv, const LabelList& labels,
           const std::vector<std::string>& owner_uids,
           const std::optional<PodViewData>& view,
           const std::optional<std::string>& event_type,
           const std::string& uid, bool has_finalizers,
           const std::string& deletion_ts,
           const std::optional<ServiceViewTuple>& service_view) {
    Blob b;
    b.rest = std::make_shared<const std::string>(blob);
    b.whole = true;
    Fields f;
    f.rv = rv; f.uid = uid; f.deletion_ts = deletion_ts;
    f.has_finalizers = has_finalizers;
    f.labels = labels; f.owner_uids = owner_uids;
    if (view) { f.has_view = true; f.view = *view; }
    if (service_view) {
      f.has_service_view = true;
      ServiceViewData& sv = f.service_view;
      sv.name = std::get<0>(*service_view);
      sv.ns = std::get<1>(*service_view);
      sv.cluster_ip = std::get<2>(*service_view);
      for (const PortTuple& t : std::get<3>(*service_view)) {
        ServicePortView pv;
        pv.name = std::get<0>(t);
        if (std::get<1>(t)) { pv.has_port = true; pv.port = *std::get<1>(t); }
        if (std::get<2>(t)) {
          pv.has_node_port = true;
          pv.node_port = *std::get<2>(t);
        }
        sv.ports.push_back(std::move(pv));
      }
    }
    return core_.put(kind, ns, name, std::move(b), std::move(f),
                     event_type ? event_type->c_str() : nullptr);
  }

  std::optional<py::bytes> fetch(const std::string& kind, const std::string& ns,
                                 const std::string& name) {
    std::optional<Blob> b = core_.fetch(kind, ns, name);
    if (!b) return std::nullopt;
    core_.note_assembled(1, b->size());
    return to_bytes(*b);
  }

  // -- tree-returning reads (json_decode.hpp) ---------------------------
  // Each hands the reader the object as json.loads of the assembled blob
  // would give it, built straight from the sections. An object the decoder
  // does not reproduce comes back as that blob (bytes) instead, for the
  // caller to json.loads: per object, so a remove never has to be repeated
  // and one odd object does not send a whole list down the slow path. Either
  // way the object counts once in blobs_assembled. The store mutex is
  // released before the first Python object is built.
  py::object decode(const Blob& b) {
    {
      kuberay_json::TreeBuilder builder;
      kuberay_json::Tokenizer<kuberay_json::TreeBuilder> tok(builder);
      const kuberay_json::Result r =
          tok.entry(b.rest.get(), b.meta.get(), b.status.get(), b.whole);
      if (r == kuberay_json::Result::kOk) {
        core_.note_decode(true);
        return py::reinterpret_steal<py::object>(builder.release());
      }
    }
    if (PyErr_Occurred()) PyErr_Clear();  // json.loads meets it again
    core_.note_decode(false);
    return to_bytes(b);
  }

  py::object fetch_tree(const std::string& kind, const std::string& ns,
                        const std::string& name) {
    std::optional<Blob> b = core_.fetch(kind, ns, name);
    if (!b) return py::none();
    core_.note_assembled(1, b->size());
    return decode(*b);
  }

  py::object remove_tree(const std::string& kind, const std::string& ns,
                         const std::string& name,
                         std::optional<int64_t> event_rv) {
    std::optional<Blob> b = core_.remove(kind, ns, name, event_rv);
    if (!b) return py::none();
    core_.note_assembled(1, b->size());
    return decode(*b);
  }

  py::list list_trees(const std::string& kind,
                      const std::optional<std::string>& ns,
                      const LabelList& selector) {
    std::vector<Blob> blobs = core_.list(kind, ns, selector);
    py::list out;
    size_t bytes = 0;
    for (const Blob& b : blobs) {
      bytes += b.size();
      out.append(decode(b));
    }
    core_.note_assembled(blobs.size(), bytes);
    return out;
  }

  // [(event type, tree or bytes, rv override or None)], as history_since.
  py::object history_since_trees(
      int64_t rv, const std::optional<std::unordered_set<std::string>>& kinds) {
    std::optional<std::vector<HistoryItem>> items =
        core_.history_since(rv, kinds ? &*kinds : nullptr);
    if (!items) return py::none();
    py::list out;
    size_t bytes = 0;
    for (const HistoryItem& h : *items) {
      bytes += h.blob.size();
      py::object override_rv = py::none();
      if (h.rv_override) override_rv = py::int_(*h.rv_override);
      out.append(py::make_tuple(h.event_type, decode(h.blob), override_rv));
    }
    core_.note_assembled(items->size(), bytes);
    return out;
  }

  std::optional<std::string> rv(const std::string& kind, const std::string& ns,
                                const std::string& name) const {
    return core_.rv(kind, ns, name);
  }

  py::object peek(const std::string& kind, const std::string& ns,
                  const std::string& name) const {
    std::optional<Peek> p = core_.peek(kind, ns, name);
    if (!p) return py::none();
    return py::make_tuple(p->rv, p->uid, p->has_finalizers, p->deletion_ts);
  }

  bool contains(const std::string& kind, const std::string& ns,
                const std::string& name) const {
    return core_.contains(kind, ns, name);
  }

  std::optional<py::bytes> remove(const std::string& kind, const std::string& ns,
                                  const std::string& name,
                                  std::optional<int64_t> event_rv) {
    std::optional<Blob> b = core_.remove(kind, ns, name, event_rv);
    if (!b) return std::nullopt;
    core_.note_assembled(1, b->size());
    return to_bytes(*b);
  }

  std::vector<py::bytes> list_blobs(const std::string& kind,
                                    const std::optional<std::string>& ns,
                                    const LabelList& selector) {
    std::vector<Blob> blobs = core_.list(kind, ns, selector);
    std::vector<py::bytes> out;
    out.reserve(blobs.size());
    size_t bytes = 0;
    for (const Blob& b : blobs) {
      bytes += b.size();
      out.push_back(to_bytes(b));
    }
    core_.note_assembled(blobs.size(), bytes);
    return out;
  }

  // Returns per-pod view tuples:
  // (name, ns, labels, phase, ready, deletion_ts, pod_ip, restart_policy,
  //  terminated, creation_ts)
  py::list list_views(const std::optional<std::string>& ns,
                      const LabelList& selector) const {
    std::vector<ViewRow> rows = core_.list_views(ns, selector);
    py::list out;
    for (const ViewRow& r : rows) {
      py::dict labels;
      for (const auto& kv : r.labels) {
        labels[py::str(kv.first)] = py::str(kv.second);
      }
      out.append(py::make_tuple(
          r.view.name, r.view.ns, labels, r.view.phase, r.view.ready,
          r.view.deletion_ts, r.view.pod_ip, r.view.restart_policy,
          r.view.terminated, r.view.creation_ts));
    }
    return out;
  }

  std::optional<ServiceViewTuple> service_view(const std::string& ns,
                                               const std::string& name) const {
    std::optional<ServiceViewData> v = core_.service_view(ns, name);
    if (!v) return std::nullopt;
    std::vector<PortTuple> ports;
    ports.reserve(v->ports.size());
    for (const ServicePortView& p : v->ports) {
      ports.emplace_back(
          p.name, p.has_port ? std::optional<int64_t>(p.port) : std::nullopt,
          p.has_node_port ? std::optional<int64_t>(p.node_port) : std::nullopt);
    }
    return ServiceViewTuple(v->name, v->ns, v->cluster_ip, std::move(ports));
  }

  std::vector<py::tuple> dependents(const std::string& uid) const {
    std::vector<py::tuple> out;
    for (const auto& t : core_.dependents(uid)) {
      out.push_back(py::make_tuple(std::get<0>(t), std::get<1>(t),
                                   std::get<2>(t)));
    }
    return out;
  }

  void drop_owner(const std::string& uid) { core_.drop_owner(uid); }
  size_t count(const std::string& kind) const { return core_.count(kind); }
  size_t total_bytes() const { return core_.total_bytes(); }

  // [(event type, bytes, rv override or None)] oldest first, or None when
  // `rv` is older than the ring can replay.
  py::object history_since(int64_t rv,
                           const std::optional<std::unordered_set<std::string>>&
                               kinds) {
    std::optional<std::vector<HistoryItem>> items =
        core_.history_since(rv, kinds ? &*kinds : nullptr);
    if (!items) return py::none();
    py::list out;
    size_t bytes = 0;
    for (const HistoryItem& h : *items) {
      bytes += h.blob.size();
      py::object override_rv = py::none();
      if (h.rv_override) override_rv = py::int_(*h.rv_override);
      out.append(py::make_tuple(h.event_type, to_bytes(h.blob), override_rv));
    }
    core_.note_assembled(items->size(), bytes);
    return out;
  }

  void history_reset(int64_t base, size_t capacity) {
    core_.history_reset(base, capacity);
  }

  std::vector<int64_t> history_rvs() const { return core_.history_rvs(); }

  py::dict stats() const {
    const Stats s = core_.stats();
    py::dict d;
    d["full_encodes"] = s.full_encodes;
    d["partial_encodes"] = s.partial_encodes;
    d["bytes_encoded"] = s.bytes_encoded;
    d["blobs_assembled"] = s.blobs_assembled;
    d["bytes_assembled"] = s.bytes_assembled;
    d["fallbacks"] = s.fallbacks;
    d["history_appends"] = s.history_appends;
    d["trees_decoded"] = s.trees_decoded;
    d["decode_fallbacks"] = s.decode_fallbacks;
    return d;
  }

 private:
  StoreCore core_;
};

}  // namespace

PYBIND11_MODULE(engine, m) {
  m.doc() = "kuberay-amd native object store (C++ sections + indexes + pod "
            "and Service views + watch history, native JSON encoding) and "
            "model-tree copier";
  init_keys();

  // Deep copy of a pydantic model tree (tree_copy.hpp). copy_configure takes
  // pydantic.BaseModel once, so the engine imports where pydantic is absent.
  m.def("copy_configure", [](py::handle base_model) {
    return kuberay_copy::configure(base_model.ptr());
  }, py::arg("base_model"),
        "Hand the copier pydantic.BaseModel; returns whether it is enabled.");
  m.def("copy_tree", [](py::handle obj) -> py::object {
    PyObject* out = kuberay_copy::copy_tree(obj.ptr());
    if (out == nullptr) return py::none();
    return py::reinterpret_steal<py::object>(out);
  }, py::arg("obj"),
        "copy.deepcopy of a model tree, or None when it declines.");
  m.def("copy_stats", []() {
    const kuberay_copy::State& s = kuberay_copy::state();
    py::dict d;
    d["copies"] = s.copies;
    d["declines"] = s.declines;
    return d;
  });

  py::class_<PodViewData>(m, "PodViewData")
      .def(py::init<>())
      .def_readwrite("name", &PodViewData::name)
      .def_readwrite("ns", &PodViewData::ns)
      .def_readwrite("phase", &PodViewData::phase)
      .def_readwrite("deletion_ts", &PodViewData::deletion_ts)
      .def_readwrite("pod_ip", &PodViewData::pod_ip)
      .def_readwrite("restart_policy", &PodViewData::restart_policy)
      .def_readwrite("creation_ts", &PodViewData::creation_ts)
      .def_readwrite("ready", &PodViewData::ready)
      .def_readwrite("terminated", &PodViewData::terminated);

  py::class_<NativeStore>(m, "NativeStore")
      .def(py::init<size_t>(), py::arg("history_capacity") = 1024)
      .def("put_object", &NativeStore::put_object, py::arg("kind"),
           py::arg("ns"), py::arg("name"), py::arg("obj"),
           py::arg("event_type") = std::nullopt)
      .def("put_status", &NativeStore::put_status, py::arg("kind"),
           py::arg("ns"), py::arg("name"), py::arg("obj"),
           py::arg("event_type") = std::nullopt)
      .def("put", &NativeStore::put, py::arg("kind"), py::arg("ns"),
           py::arg("name"), py::arg("blob"), py::arg("rv"), py::arg("labels"),
           py::arg("owner_uids"), py::arg("view") = std::nullopt,
           py::arg("event_type") = std::nullopt, py::arg("uid") = "",
           py::arg("has_finalizers") = false, py::arg("deletion_ts") = "",
           py::arg("service_view") = std::nullopt)
      .def("fetch", &NativeStore::fetch)
      .def("fetch_tree", &NativeStore::fetch_tree)
      .def("remove_tree", &NativeStore::remove_tree, py::arg("kind"),
           py::arg("ns"), py::arg("name"), py::arg("event_rv") = std::nullopt)
      .def("list_trees", &NativeStore::list_trees, py::arg("kind"),
           py::arg("ns") = std::nullopt, py::arg("selector") = LabelList())
      .def("history_since_trees", &NativeStore::history_since_trees,
           py::arg("rv"), py::arg("kinds") = std::nullopt)
      .def("rv", &NativeStore::rv)
      .def("peek", &NativeStore::peek)
      .def("contains", &NativeStore::contains)
      .def("remove", &NativeStore::remove, py::arg("kind"), py::arg("ns"),
           py::arg("name"), py::arg("event_rv") = std::nullopt)
      .def("list_blobs", &NativeStore::list_blobs, py::arg("kind"),
           py::arg("ns") = std::nullopt, py::arg("selector") = LabelList())
      .def("list_views", &NativeStore::list_views, py::arg("ns") = std::nullopt,
           py::arg("selector") = LabelList())
      .def("service_view", &NativeStore::service_view)
      .def("dependents", &NativeStore::dependents)
      .def("drop_owner", &NativeStore::drop_owner)
      .def("count", &NativeStore::count)
      .def("total_bytes", &NativeStore::total_bytes)
      .def("history_since", &NativeStore::history_since, py::arg("rv"),
           py::arg("kinds") = std::nullopt)
      .def("history_reset", &NativeStore::history_reset, py::arg("base"),
           py::arg("capacity") = 0)
      .def("history_rvs", &NativeStore::history_rvs)
      .def("stats", &NativeStore::stats);
}
