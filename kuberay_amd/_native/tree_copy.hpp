// tree_copy — deep copy of a pydantic model tree without the interpreter.
//
// The operator clones pod templates, built pods and cluster specs several
// times per reconcile. copy.deepcopy pays the copy module's dispatch and memo
// per node and runs BaseModel.__deepcopy__ in Python per model; for a built
// worker pod (242 nodes, 38 models) that costs more than building the pod.
// This copier walks the same tree with the C API and gives exactly what
// copy.deepcopy gives, or nothing: anything it does not reproduce exactly
// declines the whole call, the partial copy is dropped, and the caller
// (K8sModel.clone) runs copy.deepcopy as before.
//
// Accepted nodes: None, bool, exact int / float / str (shared, as deepcopy
// shares them), exact dict with exact-str keys, exact list, and instances of
// pydantic.BaseModel whose __deepcopy__ is BaseModel's own, whose
// __pydantic_private__ is None, whose __pydantic_extra__ is None or an exact
// dict and whose __pydantic_fields_set__ is an exact set. A model is copied
// the way BaseModel.__deepcopy__ copies it: tp_new (no __init__, no
// validation), deep copies of __dict__ and __pydantic_extra__, a shallow copy
// of __pydantic_fields_set__, __pydantic_private__ = None, all four set the
// way object.__setattr__ sets them. Values are copied for what they are, not
// for what the field annotation says.
//
// Two references to one dict, list or model in the source are one object in
// the copy (deepcopy's memo). A dict or list that contains itself is
// reproduced; a model reached again while it is being copied declines.
//
// The GIL is held throughout, nothing is kept past the call, and a Python
// error part-way (out of memory, a __new__ that raises) is cleared and turned
// into a decline, so the fallback meets and reports it as it always did.
#pragma once

#include <Python.h>

#include <cstdint>
#include <cstring>
#include <vector>

namespace kuberay_copy {

// Containers nested deeper than this decline (a model counts twice: itself
// and its __dict__). deepcopy goes on to the interpreter's recursion limit.
constexpr int kMaxDepth = 128;

struct State {
  PyObject* base_model = nullptr;     // pydantic.BaseModel
  PyObject* base_deepcopy = nullptr;  // BaseModel.__dict__['__deepcopy__']
  PyObject *s_dict = nullptr, *s_fields_set = nullptr, *s_extra = nullptr,
           *s_private = nullptr, *s_deepcopy = nullptr;
  PyObject* empty_tuple = nullptr;
  uint64_t copies = 0, declines = 0;  // guarded by the GIL
};

inline State& state() {
  static State s;
  return s;
}

// Takes pydantic.BaseModel (or None to disable). Returns whether the copier
// is enabled: BaseModel must carry __deepcopy__ and the four slots
// BaseModel.__deepcopy__ writes; otherwise every copy_tree call declines.
inline bool configure(PyObject* base_model) {
  State& s = state();
  Py_CLEAR(s.base_model);
  Py_CLEAR(s.base_deepcopy);
  if (s.s_dict == nullptr) {
    s.s_dict = PyUnicode_InternFromString("__dict__");
    s.s_fields_set = PyUnicode_InternFromString("__pydantic_fields_set__");
    s.s_extra = PyUnicode_InternFromString("__pydantic_extra__");
    s.s_private = PyUnicode_InternFromString("__pydantic_private__");
    s.s_deepcopy = PyUnicode_InternFromString("__deepcopy__");
    s.empty_tuple = PyTuple_New(0);
  }
  if (base_model == nullptr || base_model == Py_None) return false;
  if (!PyType_Check(base_model)) return false;
  PyObject* tp_dict = reinterpret_cast<PyTypeObject*>(base_model)->tp_dict;
  if (tp_dict == nullptr) return false;
  for (PyObject* name : {s.s_dict, s.s_fields_set, s.s_extra, s.s_private}) {
    PyObject* descr = PyDict_GetItemWithError(tp_dict, name);
    if (descr == nullptr || Py_TYPE(descr)->tp_descr_get == nullptr ||
        Py_TYPE(descr)->tp_descr_set == nullptr) {
      PyErr_Clear();
      return false;
    }
  }
  PyObject* dc = PyDict_GetItemWithError(tp_dict, s.s_deepcopy);
  if (dc == nullptr) {
    PyErr_Clear();
    return false;
  }
  Py_INCREF(base_model);
  s.base_model = base_model;
  Py_INCREF(dc);
  s.base_deepcopy = dc;
  return true;
}

// source container -> its copy (borrowed: the copy is owned by the tree under
// construction). nullptr marks a model whose copy is still being built.
class Memo {
 public:
  Memo() : cap_(kInline), n_(0), keys_(k0_), vals_(v0_) {
    std::memset(k0_, 0, sizeof k0_);
  }

  // Slot for `key`: *found says whether it was already there.
  PyObject** slot(PyObject* key, bool* found) {
    if ((n_ + 1) * 2 > cap_) grow();
    size_t i = hash(key) & (cap_ - 1);
    while (keys_[i] != nullptr) {
      if (keys_[i] == key) {
        *found = true;
        return &vals_[i];
      }
      i = (i + 1) & (cap_ - 1);
    }
    *found = false;
    keys_[i] = key;
    vals_[i] = nullptr;
    ++n_;
    return &vals_[i];
  }

  void set(PyObject* key, PyObject* val) {
    bool found;
    *slot(key, &found) = val;
  }

 private:
  static constexpr size_t kInline = 256;

  static size_t hash(PyObject* p) {
    return static_cast<size_t>(
        (reinterpret_cast<uintptr_t>(p) >> 4) * 0x9E3779B97F4A7C15ull >> 20);
  }

  void grow() {
    const size_t ncap = cap_ * 2;
    std::vector<PyObject*> nk(ncap, nullptr), nv(ncap, nullptr);
    for (size_t i = 0; i < cap_; ++i) {
      if (keys_[i] == nullptr) continue;
      size_t j = hash(keys_[i]) & (ncap - 1);
      while (nk[j] != nullptr) j = (j + 1) & (ncap - 1);
      nk[j] = keys_[i];
      nv[j] = vals_[i];
    }
    hk_.swap(nk);
    hv_.swap(nv);
    keys_ = hk_.data();
    vals_ = hv_.data();
    cap_ = ncap;
  }

  size_t cap_, n_;
  PyObject** keys_;
  PyObject** vals_;
  PyObject* k0_[kInline];
  PyObject* v0_[kInline];
  std::vector<PyObject*> hk_, hv_;
};

// Every function below returns a new reference, or nullptr for a decline
// (no Python error is left set).
inline PyObject* copy_node(Memo& memo, PyObject* o, int depth);

inline bool is_leaf(PyObject* o) {
  PyTypeObject* tp = Py_TYPE(o);
  return tp == &PyUnicode_Type || o == Py_None || tp == &PyBool_Type ||
         tp == &PyLong_Type || tp == &PyFloat_Type;
}

inline PyObject* copy_dict(Memo& memo, PyObject* d, int depth) {
  if (depth >= kMaxDepth) return nullptr;
  // One C-level copy carries keys, order and every leaf value; only values
  // that are containers are then replaced by their copies.
  PyObject* out = PyDict_Copy(d);
  if (out == nullptr) {
    PyErr_Clear();
    return nullptr;
  }
  memo.set(d, out);
  Py_ssize_t pos = 0;
  PyObject *k, *v;
  while (PyDict_Next(d, &pos, &k, &v)) {
    if (!PyUnicode_CheckExact(k)) {
      Py_DECREF(out);
      return nullptr;
    }
    if (is_leaf(v)) continue;
    PyObject* c = copy_node(memo, v, depth + 1);
    if (c == nullptr) {
      Py_DECREF(out);
      return nullptr;
    }
    const int rc = PyDict_SetItem(out, k, c);
    Py_DECREF(c);
    if (rc < 0) {
      PyErr_Clear();
      Py_DECREF(out);
      return nullptr;
    }
  }
  return out;
}

inline PyObject* copy_list(Memo& memo, PyObject* l, int depth) {
  if (depth >= kMaxDepth) return nullptr;
  const Py_ssize_t n = PyList_GET_SIZE(l);
  PyObject* out = PyList_New(n);
  if (out == nullptr) {
    PyErr_Clear();
    return nullptr;
  }
  memo.set(l, out);
  for (Py_ssize_t i = 0; i < n; ++i) {
    PyObject* c = i < PyList_GET_SIZE(l)
                      ? copy_node(memo, PyList_GET_ITEM(l, i), depth + 1)
                      : nullptr;
    if (c == nullptr) {
      Py_DECREF(out);
      return nullptr;
    }
    PyList_SET_ITEM(out, i, c);
  }
  return out;
}

// getattr for one of the four slots; an unset slot (AttributeError) is
// nullptr with the error cleared
inline PyObject* slot_get(PyObject* o, PyObject* name) {
  PyObject* v = PyObject_GenericGetAttr(o, name);
  if (v == nullptr) PyErr_Clear();
  return v;
}

inline PyObject* copy_model(Memo& memo, PyObject* o, int depth) {
  if (depth >= kMaxDepth) return nullptr;
  State& s = state();
  PyTypeObject* tp = Py_TYPE(o);
  if (_PyType_Lookup(tp, s.s_deepcopy) != s.base_deepcopy) return nullptr;
  if (tp->tp_new == nullptr) return nullptr;

  PyObject *priv = nullptr, *extra = nullptr, *fields_set = nullptr,
           *dict = nullptr;
  PyObject *m = nullptr, *ndict = nullptr, *nextra = nullptr, *nset = nullptr;
  bool ok = false;
  do {
    priv = slot_get(o, s.s_private);
    if (priv != Py_None) break;
    extra = slot_get(o, s.s_extra);
    if (extra == nullptr || (extra != Py_None && !PyDict_CheckExact(extra))) break;
    fields_set = slot_get(o, s.s_fields_set);
    if (fields_set == nullptr || Py_TYPE(fields_set) != &PySet_Type) break;
    dict = slot_get(o, s.s_dict);
    if (dict == nullptr || !PyDict_CheckExact(dict)) break;

    m = tp->tp_new(tp, s.empty_tuple, nullptr);
    if (m == nullptr) {
      PyErr_Clear();
      break;
    }
    if (Py_TYPE(m) != tp) break;

    bool found;
    PyObject* hit;
    hit = *memo.slot(dict, &found);
    if (found) {
      if (hit == nullptr) break;
      ndict = hit;
      Py_INCREF(ndict);
    } else {
      ndict = copy_dict(memo, dict, depth + 1);
      if (ndict == nullptr) break;
    }
    if (extra == Py_None) {
      nextra = Py_None;
      Py_INCREF(nextra);
    } else {
      hit = *memo.slot(extra, &found);
      if (found) {
        if (hit == nullptr) break;
        nextra = hit;
        Py_INCREF(nextra);
      } else {
        nextra = copy_dict(memo, extra, depth + 1);
        if (nextra == nullptr) break;
      }
    }
    nset = PySet_New(fields_set);
    if (nset == nullptr) {
      PyErr_Clear();
      break;
    }
    if (PyObject_GenericSetAttr(m, s.s_dict, ndict) < 0 ||
        PyObject_GenericSetAttr(m, s.s_extra, nextra) < 0 ||
        PyObject_GenericSetAttr(m, s.s_fields_set, nset) < 0 ||
        PyObject_GenericSetAttr(m, s.s_private, Py_None) < 0) {
      PyErr_Clear();
      break;
    }
    ok = true;
  } while (false);

  Py_XDECREF(priv); Py_XDECREF(extra); Py_XDECREF(fields_set); Py_XDECREF(dict);
  Py_XDECREF(ndict); Py_XDECREF(nextra); Py_XDECREF(nset);
  if (!ok) {
    Py_XDECREF(m);
    return nullptr;
  }
  return m;
}

inline PyObject* copy_node(Memo& memo, PyObject* o, int depth) {
  if (is_leaf(o)) {
    Py_INCREF(o);
    return o;
  }
  PyTypeObject* tp = Py_TYPE(o);
  const bool is_dict = tp == &PyDict_Type, is_list = tp == &PyList_Type;
  if (!is_dict && !is_list &&
      !PyType_IsSubtype(tp, reinterpret_cast<PyTypeObject*>(state().base_model))) {
    return nullptr;  // tuple, set, subclass of a builtin, Enum member, ...
  }
  bool found;
  PyObject** slot = memo.slot(o, &found);
  if (found) {
    PyObject* hit = *slot;
    if (hit == nullptr) return nullptr;  // a model inside itself
    Py_INCREF(hit);
    return hit;
  }
  if (is_dict) return copy_dict(memo, o, depth);
  if (is_list) return copy_list(memo, o, depth);
  // `slot` may move when the table grows: the in-progress mark it holds is
  // found again by key once the copy is done
  PyObject* m = copy_model(memo, o, depth);
  if (m != nullptr) memo.set(o, m);
  return m;
}

// The entry point: a new reference to the copy, or nullptr for a decline
// (counted; no Python error set).
inline PyObject* copy_tree(PyObject* root) {
  State& s = state();
  if (s.base_model == nullptr) {
    ++s.declines;
    return nullptr;
  }
  Memo memo;
  PyObject* out = copy_node(memo, root, 0);
  if (out == nullptr) {
    ++s.declines;
  } else {
    ++s.copies;
  }
  return out;
}

}  // namespace kuberay_copy
