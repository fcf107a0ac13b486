// store_core — the Python-free half of the native object store.
//
// Everything here is plain C++17: entries, the kind / label / owner-uid
// indexes, the pod and Service views, the three shared JSON sections of every
// object, the watch history ring and the work counters. engine.cpp adds the pybind11 bindings and the
// PyObject encoder on top; tests/native/store_core_check.cpp drives this
// header alone (under sanitizers).
//
// An object is kept as up to three immutable, independently shared pieces of
// compact JSON:
//   rest   — every top-level member except "metadata" and "status", already
//            joined as `"k":v,"k":v` (no braces),
//   meta   — the value of "metadata" (absent if the object has none),
//   status — the value of "status" (absent if the object has none).
// A status write replaces meta + status and keeps the rest pointer; a history
// entry holds the same pointers, so nothing is ever encoded or copied twice.
// An entry written from a ready-made blob ("whole") keeps that blob in `rest`.
//
// Thread-safe via one internal mutex. No call holds it while it builds or
// returns anything bigger than a handful of shared_ptr copies.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <tuple>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

namespace kuberay_store {

using Section = std::shared_ptr<const std::string>;
using LabelList = std::vector<std::pair<std::string, std::string>>;

struct PodViewData {
  std::string name, ns, phase, deletion_ts, pod_ip, restart_policy, creation_ts;
  bool ready = false;
  bool terminated = false;
};

// What the RayCluster reconciler reads from a Service: whether it exists,
// its clusterIP ("" when it has none) and (name, port, nodePort) per port.
// A port number the object does not carry has its flag false.
struct ServicePortView {
  std::string name;
  int64_t port = 0, node_port = 0;
  bool has_port = false, has_node_port = false;
};

struct ServiceViewData {
  std::string name, ns, cluster_ip;
  std::vector<ServicePortView> ports;
};

// The stored form of one object version.
struct Blob {
  Section rest, meta, status;
  bool whole = false;  // rest is a complete JSON document

  size_t size() const {
    if (whole) return rest ? rest->size() : 0;
    size_t n = 2;  // braces
    bool first = true;
    if (rest && !rest->empty()) { n += rest->size(); first = false; }
    if (meta) { n += (first ? 0 : 1) + 11 + meta->size(); first = false; }
    if (status) { n += (first ? 0 : 1) + 9 + status->size(); }
    return n;
  }

  // Writes exactly size() bytes.
  void write(char* out) const {
    if (whole) {
      if (rest) std::memcpy(out, rest->data(), rest->size());
      return;
    }
    *out++ = '{';
    bool first = true;
    if (rest && !rest->empty()) {
      std::memcpy(out, rest->data(), rest->size());
      out += rest->size();
      first = false;
    }
    if (meta) {
      if (!first) *out++ = ',';
      std::memcpy(out, "\"metadata\":", 11); out += 11;
      std::memcpy(out, meta->data(), meta->size()); out += meta->size();
      first = false;
    }
    if (status) {
      if (!first) *out++ = ',';
      std::memcpy(out, "\"status\":", 9); out += 9;
      std::memcpy(out, status->data(), status->size()); out += status->size();
    }
    *out = '}';
  }

  std::string str() const {
    std::string s(size(), '\0');
    write(s.data());
    return s;
  }
};

// What a write extracts from metadata (and, for pods, spec + status).
struct Fields {
  std::string rv, uid, deletion_ts;
  bool has_finalizers = false;
  LabelList labels;
  std::vector<std::string> owner_uids;
  bool has_view = false;
  PodViewData view;
  // Services only. A status write keeps it: everything in it comes from
  // spec and from metadata a status write cannot change.
  bool has_service_view = false;
  ServiceViewData service_view;
};

struct Peek {
  std::string rv, uid, deletion_ts;
  bool has_finalizers = false;
};

struct ViewRow {
  PodViewData view;
  LabelList labels;
};

struct HistoryItem {
  std::string event_type;
  Blob blob;
  std::optional<int64_t> rv_override;  // set on DELETED
};

struct Stats {
  uint64_t full_encodes = 0, partial_encodes = 0, bytes_encoded = 0;
  uint64_t blobs_assembled = 0, bytes_assembled = 0;
  uint64_t fallbacks = 0, history_appends = 0;
  uint64_t trees_decoded = 0, decode_fallbacks = 0;
};

inline std::string make_key(const std::string& kind, const std::string& ns,
                            const std::string& name) {
  std::string k;
  k.reserve(kind.size() + ns.size() + name.size() + 2);
  k += kind; k += '\x1f'; k += ns; k += '\x1f'; k += name;
  return k;
}

inline std::string label_key(const std::string& kind, const std::string& k,
                             const std::string& v) {
  std::string out;
  out.reserve(kind.size() + k.size() + v.size() + 2);
  out += kind; out += '\x1f'; out += k; out += '\x1f'; out += v;
  return out;
}

class StoreCore {
 public:
  explicit StoreCore(size_t history_capacity = 1024)
      : ring_(history_capacity ? history_capacity : 1) {}

  // Full write. `event_type` non-null appends the history entry in the same
  // critical section. Returns true when the key was new.
  bool put(const std::string& kind, const std::string& ns,
           const std::string& name, Blob blob, Fields f,
           const char* event_type) {
    std::lock_guard<std::mutex> g(mu_);
    std::string key = make_key(kind, ns, name);
    auto it = objects_.find(key);
    const bool is_new = it == objects_.end();
    if (!is_new) index_remove(key, it->second);
    Entry e;
    e.kind = kind; e.ns = ns; e.name = name;
    e.blob = std::move(blob);
    e.f = std::move(f);
    index_add(key, e);
    if (event_type) history_append(event_type, kind, e.blob, e.f.rv, false);
    if (is_new) {
      objects_.emplace(std::move(key), std::move(e));
    } else {
      it->second = std::move(e);
    }
    return is_new;
  }

  // Status write: swaps meta + status, keeps rest and the label / owner
  // indexes. Returns false (and changes nothing) when the key is missing or
  // the entry is a whole blob that cannot be spliced.
  bool put_status(const std::string& kind, const std::string& ns,
                  const std::string& name, Section meta, Section status,
                  Peek p, bool has_view, PodViewData view,
                  const char* event_type) {
    std::lock_guard<std::mutex> g(mu_);
    auto it = objects_.find(make_key(kind, ns, name));
    if (it == objects_.end() || it->second.blob.whole) return false;
    Entry& e = it->second;
    e.blob.meta = std::move(meta);
    e.blob.status = std::move(status);
    e.f.rv = std::move(p.rv);
    e.f.uid = std::move(p.uid);
    e.f.deletion_ts = std::move(p.deletion_ts);
    e.f.has_finalizers = p.has_finalizers;
    e.f.has_view = has_view;
    e.f.view = std::move(view);
    if (event_type) history_append(event_type, kind, e.blob, e.f.rv, false);
    return true;
  }

  std::optional<Blob> fetch(const std::string& kind, const std::string& ns,
                            const std::string& name) const {
    std::lock_guard<std::mutex> g(mu_);
    auto it = objects_.find(make_key(kind, ns, name));
    if (it == objects_.end()) return std::nullopt;
    return it->second.blob;
  }

  std::optional<std::string> rv(const std::string& kind, const std::string& ns,
                                const std::string& name) const {
    std::lock_guard<std::mutex> g(mu_);
    auto it = objects_.find(make_key(kind, ns, name));
    if (it == objects_.end()) return std::nullopt;
    return it->second.f.rv;
  }

  std::optional<Peek> peek(const std::string& kind, const std::string& ns,
                           const std::string& name) const {
    std::lock_guard<std::mutex> g(mu_);
    auto it = objects_.find(make_key(kind, ns, name));
    if (it == objects_.end()) return std::nullopt;
    const Fields& f = it->second.f;
    Peek p;
    p.rv = f.rv; p.uid = f.uid; p.deletion_ts = f.deletion_ts;
    p.has_finalizers = f.has_finalizers;
    return p;
  }

  bool contains(const std::string& kind, const std::string& ns,
                const std::string& name) const {
    std::lock_guard<std::mutex> g(mu_);
    return objects_.count(make_key(kind, ns, name)) != 0;
  }

  // With `event_rv`, the DELETED history entry points at the removed
  // sections and carries that rv beside them.
  std::optional<Blob> remove(const std::string& kind, const std::string& ns,
                             const std::string& name,
                             std::optional<int64_t> event_rv = std::nullopt) {
    std::lock_guard<std::mutex> g(mu_);
    auto it = objects_.find(make_key(kind, ns, name));
    if (it == objects_.end()) return std::nullopt;
    Blob out = std::move(it->second.blob);
    index_remove(it->first, it->second);
    objects_.erase(it);
    if (event_rv) {
      append_raw(*event_rv, "DELETED", kind, out, true);
    }
    return out;
  }

  std::vector<Blob> list(const std::string& kind,
                         const std::optional<std::string>& ns,
                         const LabelList& selector) const {
    std::lock_guard<std::mutex> g(mu_);
    std::vector<const Entry*> entries = select(kind, ns, selector);
    std::vector<Blob> out;
    out.reserve(entries.size());
    for (const Entry* e : entries) out.push_back(e->blob);
    return out;
  }

  std::vector<ViewRow> list_views(const std::optional<std::string>& ns,
                                  const LabelList& selector) const {
    std::lock_guard<std::mutex> g(mu_);
    std::vector<const Entry*> entries = select("Pod", ns, selector);
    std::vector<ViewRow> out;
    out.reserve(entries.size());
    for (const Entry* e : entries) {
      if (!e->f.has_view) continue;
      out.push_back(ViewRow{e->f.view, e->f.labels});
    }
    return out;
  }

  // The view of Service ns/name; nullopt when there is no such Service or
  // its last full write produced no view.
  std::optional<ServiceViewData> service_view(const std::string& ns,
                                              const std::string& name) const {
    std::lock_guard<std::mutex> g(mu_);
    auto it = objects_.find(make_key("Service", ns, name));
    if (it == objects_.end() || !it->second.f.has_service_view) {
      return std::nullopt;
    }
    return it->second.f.service_view;
  }

  std::vector<std::tuple<std::string, std::string, std::string>> dependents(
      const std::string& uid) const {
    std::lock_guard<std::mutex> g(mu_);
    std::vector<std::tuple<std::string, std::string, std::string>> out;
    auto it = owner_index_.find(uid);
    if (it == owner_index_.end()) return out;
    for (const auto& key : it->second) {
      auto oit = objects_.find(key);
      if (oit != objects_.end()) {
        out.emplace_back(oit->second.kind, oit->second.ns, oit->second.name);
      }
    }
    return out;
  }

  void drop_owner(const std::string& uid) {
    std::lock_guard<std::mutex> g(mu_);
    owner_index_.erase(uid);
  }

  size_t count(const std::string& kind) const {
    std::lock_guard<std::mutex> g(mu_);
    auto it = kind_index_.find(kind);
    return it == kind_index_.end() ? 0 : it->second.size();
  }

  // Bytes held by live objects; every section counted once.
  size_t total_bytes() const {
    std::lock_guard<std::mutex> g(mu_);
    std::unordered_set<const std::string*> seen;
    size_t n = 0;
    auto add = [&](const Section& s) {
      if (s && seen.insert(s.get()).second) n += s->size();
    };
    for (const auto& kv : objects_) {
      add(kv.second.blob.rest);
      add(kv.second.blob.meta);
      add(kv.second.blob.status);
    }
    return n;
  }

  // -- history ring ----------------------------------------------------
  // Events with rv > `rv`, oldest first; nullopt when `rv` predates what the
  // ring can prove complete (below base, or ring full and oldest > rv + 1).
  std::optional<std::vector<HistoryItem>> history_since(
      int64_t rv, const std::unordered_set<std::string>* kinds) const {
    std::lock_guard<std::mutex> g(mu_);
    if (rv < base_) return std::nullopt;
    if (ring_len_ == ring_.size() && ring_[ring_head_].rv > rv + 1) {
      return std::nullopt;
    }
    std::vector<HistoryItem> out;
    for (size_t i = 0; i < ring_len_; ++i) {
      const HistEntry& h = ring_[(ring_head_ + i) % ring_.size()];
      if (h.rv <= rv) continue;
      if (kinds && kinds->count(h.kind) == 0) continue;
      HistoryItem item;
      item.event_type = h.event_type;
      item.blob = h.blob;
      if (h.override_rv) item.rv_override = h.rv;
      out.push_back(std::move(item));
    }
    return out;
  }

  // Snapshot restore: drop every entry and refuse replays below `base`.
  // A non-zero `capacity` also resizes the ring.
  void history_reset(int64_t base, size_t capacity = 0) {
    std::vector<HistEntry> old;
    {
      std::lock_guard<std::mutex> g(mu_);
      old.swap(ring_);
      ring_.assign(capacity ? capacity : old.size(), HistEntry{});
      ring_head_ = ring_len_ = 0;
      base_ = base;
      last_rv_ = std::max(last_rv_, base);
    }
  }

  size_t history_size() const {
    std::lock_guard<std::mutex> g(mu_);
    return ring_len_;
  }

  // rvs of the retained entries, oldest first (tests).
  std::vector<int64_t> history_rvs() const {
    std::lock_guard<std::mutex> g(mu_);
    std::vector<int64_t> out;
    out.reserve(ring_len_);
    for (size_t i = 0; i < ring_len_; ++i) {
      out.push_back(ring_[(ring_head_ + i) % ring_.size()].rv);
    }
    return out;
  }

  // -- counters --------------------------------------------------------
  void note_encode(bool full, size_t bytes) {
    (full ? full_encodes_ : partial_encodes_).fetch_add(1, std::memory_order_relaxed);
    bytes_encoded_.fetch_add(bytes, std::memory_order_relaxed);
  }
  void note_assembled(size_t blobs, size_t bytes) {
    blobs_assembled_.fetch_add(blobs, std::memory_order_relaxed);
    bytes_assembled_.fetch_add(bytes, std::memory_order_relaxed);
  }
  void note_fallback() { fallbacks_.fetch_add(1, std::memory_order_relaxed); }
  // A read handed out as a tree built from the sections / as bytes for
  // json.loads because the decoder does not reproduce the object.
  void note_decode(bool decoded) {
    (decoded ? trees_decoded_ : decode_fallbacks_)
        .fetch_add(1, std::memory_order_relaxed);
  }

  Stats stats() const {
    Stats s;
    s.full_encodes = full_encodes_.load(std::memory_order_relaxed);
    s.partial_encodes = partial_encodes_.load(std::memory_order_relaxed);
    s.bytes_encoded = bytes_encoded_.load(std::memory_order_relaxed);
    s.blobs_assembled = blobs_assembled_.load(std::memory_order_relaxed);
    s.bytes_assembled = bytes_assembled_.load(std::memory_order_relaxed);
    s.fallbacks = fallbacks_.load(std::memory_order_relaxed);
    s.history_appends = history_appends_.load(std::memory_order_relaxed);
    s.trees_decoded = trees_decoded_.load(std::memory_order_relaxed);
    s.decode_fallbacks = decode_fallbacks_.load(std::memory_order_relaxed);
    return s;
  }

 private:
  struct Entry {
    std::string kind, ns, name;
    Blob blob;
    Fields f;
  };

  struct HistEntry {
    int64_t rv = 0;
    bool override_rv = false;
    std::string event_type, kind;
    Blob blob;
  };

  // mu_ held. The entry's rv is the object's resourceVersion; one that does
  // not parse falls back to the newest rv seen so far.
  void history_append(const char* event_type, const std::string& kind,
                      const Blob& blob, const std::string& rv_text,
                      bool override_rv) {
    int64_t rv = last_rv_;
    if (!rv_text.empty() && rv_text.size() <= 18) {
      int64_t v = 0;
      bool ok = true;
      for (char c : rv_text) {
        if (c < '0' || c > '9') { ok = false; break; }
        v = v * 10 + (c - '0');
      }
      if (ok) rv = v;
    }
    append_raw(rv, event_type, kind, blob, override_rv);
  }

  void append_raw(int64_t rv, const char* event_type, const std::string& kind,
                  const Blob& blob, bool override_rv) {
    size_t slot;
    if (ring_len_ < ring_.size()) {
      slot = (ring_head_ + ring_len_) % ring_.size();
      ++ring_len_;
    } else {
      slot = ring_head_;
      ring_head_ = (ring_head_ + 1) % ring_.size();
    }
    HistEntry& h = ring_[slot];
    h.rv = rv;
    h.override_rv = override_rv;
    h.event_type = event_type;
    h.kind = kind;
    h.blob = blob;
    last_rv_ = std::max(last_rv_, rv);
    history_appends_.fetch_add(1, std::memory_order_relaxed);
  }

  // mu_ held. Matching entries sorted by (ns, name).
  std::vector<const Entry*> select(const std::string& kind,
                                   const std::optional<std::string>& ns,
                                   const LabelList& selector) const {
    std::vector<const Entry*> out;
    const std::unordered_set<std::string>* keys = nullptr;
    if (!selector.empty()) {
      // start from the smallest label bucket
      const std::unordered_set<std::string>* smallest = nullptr;
      for (const auto& kv : selector) {
        auto it = label_index_.find(label_key(kind, kv.first, kv.second));
        if (it == label_index_.end()) return out;  // empty bucket -> no match
        if (smallest == nullptr || it->second.size() < smallest->size()) {
          smallest = &it->second;
        }
      }
      keys = smallest;
    } else {
      auto it = kind_index_.find(kind);
      if (it == kind_index_.end()) return out;
      keys = &it->second;
    }
    for (const auto& key : *keys) {
      auto oit = objects_.find(key);
      if (oit == objects_.end()) continue;
      const Entry& e = oit->second;
      if (e.kind != kind) continue;
      if (ns && e.ns != *ns) continue;
      bool ok = true;
      for (const auto& kv : selector) {
        bool found = false;
        for (const auto& lv : e.f.labels) {
          if (lv.first == kv.first && lv.second == kv.second) { found = true; break; }
        }
        if (!found) { ok = false; break; }
      }
      if (ok) out.push_back(&e);
    }
    std::sort(out.begin(), out.end(), [](const Entry* a, const Entry* b) {
      return std::tie(a->ns, a->name) < std::tie(b->ns, b->name);
    });
    return out;
  }

  void index_add(const std::string& key, const Entry& e) {
    kind_index_[e.kind].insert(key);
    for (const auto& kv : e.f.labels) {
      label_index_[label_key(e.kind, kv.first, kv.second)].insert(key);
    }
    for (const auto& uid : e.f.owner_uids) owner_index_[uid].insert(key);
  }

  void index_remove(const std::string& key, const Entry& e) {
    auto kit = kind_index_.find(e.kind);
    if (kit != kind_index_.end()) kit->second.erase(key);
    for (const auto& kv : e.f.labels) {
      auto lit = label_index_.find(label_key(e.kind, kv.first, kv.second));
      if (lit != label_index_.end()) {
        lit->second.erase(key);
        if (lit->second.empty()) label_index_.erase(lit);
      }
    }
    for (const auto& uid : e.f.owner_uids) {
      auto oit = owner_index_.find(uid);
      if (oit != owner_index_.end()) oit->second.erase(key);
    }
  }

  mutable std::mutex mu_;
  std::unordered_map<std::string, Entry> objects_;
  std::unordered_map<std::string, std::unordered_set<std::string>> kind_index_;
  std::unordered_map<std::string, std::unordered_set<std::string>> label_index_;
  std::unordered_map<std::string, std::unordered_set<std::string>> owner_index_;

  std::vector<HistEntry> ring_;
  size_t ring_head_ = 0, ring_len_ = 0;
  int64_t base_ = 0;
  int64_t last_rv_ = 0;

  std::atomic<uint64_t> full_encodes_{0}, partial_encodes_{0}, bytes_encoded_{0};
  std::atomic<uint64_t> blobs_assembled_{0}, bytes_assembled_{0};
  std::atomic<uint64_t> fallbacks_{0}, history_appends_{0};
  std::atomic<uint64_t> trees_decoded_{0}, decode_fallbacks_{0};
};

}  // namespace kuberay_store
