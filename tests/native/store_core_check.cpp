// Stand-alone driver for kuberay_amd/_native/store_core.hpp (no Python).
// Built and run by tests/test_store_core_sanitizers.py under
// -fsanitize=address,undefined and again under -fsanitize=thread.
// Exits 0 when every check holds; prints the failed check and exits 1
// otherwise.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "store_core.hpp"

using namespace kuberay_store;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__,         \
                   __LINE__, #cond);                                      \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

static Section sec(const std::string& s) {
  return std::make_shared<const std::string>(s);
}

static Blob make_blob(const std::string& rest, const std::string& meta,
                      const char* status) {
  Blob b;
  b.rest = sec(rest);
  b.meta = sec(meta);
  if (status) b.status = sec(status);
  return b;
}

static Fields make_fields(int64_t rv, const std::string& uid,
                          const std::string& label,
                          const std::string& owner = "") {
  Fields f;
  f.rv = std::to_string(rv);
  f.uid = uid;
  f.labels.emplace_back("g", label);
  if (!owner.empty()) f.owner_uids.push_back(owner);
  return f;
}

static void single_threaded() {
  StoreCore core(8);

  // put + assembly
  bool is_new = core.put("Pod", "d", "a",
                         make_blob("\"kind\":\"Pod\",\"spec\":{\"x\":1}",
                                   "{\"name\":\"a\"}", "{\"phase\":\"P\"}"),
                         make_fields(1, "u-a", "x"), "ADDED");
  CHECK(is_new);
  CHECK(core.fetch("Pod", "d", "a")->str() ==
        "{\"kind\":\"Pod\",\"spec\":{\"x\":1},\"metadata\":{\"name\":\"a\"},"
        "\"status\":{\"phase\":\"P\"}}");
  CHECK(!core.put("Pod", "d", "a",
                  make_blob("\"kind\":\"Pod\"", "{\"name\":\"a\"}", nullptr),
                  make_fields(2, "u-a", "y"), "MODIFIED"));
  CHECK(core.fetch("Pod", "d", "a")->str() ==
        "{\"kind\":\"Pod\",\"metadata\":{\"name\":\"a\"}}");
  CHECK(core.count("Pod") == 1);
  CHECK(core.list("Pod", std::nullopt, {{"g", "x"}}).empty());
  CHECK(core.list("Pod", std::string("d"), {{"g", "y"}}).size() == 1);

  // empty rest / no metadata / whole blob
  Blob only_status;
  only_status.rest = sec("");
  only_status.status = sec("null");
  CHECK(only_status.str() == "{\"status\":null}");
  Blob empty;
  empty.rest = sec("");
  CHECK(empty.str() == "{}");
  Blob whole;
  whole.rest = sec("{\"k\":[1,2]}");
  whole.whole = true;
  core.put("Secret", "d", "w", whole, make_fields(3, "u-w", "x"), nullptr);
  CHECK(core.fetch("Secret", "d", "w")->str() == "{\"k\":[1,2]}");
  Peek p;
  p.rv = "4";
  CHECK(!core.put_status("Secret", "d", "w", sec("{}"), sec("{}"), p, false,
                         PodViewData{}, "MODIFIED"));  // cannot splice
  CHECK(!core.put_status("Secret", "d", "missing", sec("{}"), sec("{}"), p,
                         false, PodViewData{}, "MODIFIED"));

  // status splice keeps the rest pointer and the label index
  Blob before = *core.fetch("Pod", "d", "a");
  PodViewData view;
  view.name = "a"; view.ns = "d"; view.phase = "Running"; view.ready = true;
  p.rv = "5"; p.uid = "u-a";
  CHECK(core.put_status("Pod", "d", "a", sec("{\"name\":\"a\",\"rv\":5}"),
                        sec("{\"phase\":\"Running\"}"), p, true, view,
                        "MODIFIED"));
  Blob after = *core.fetch("Pod", "d", "a");
  CHECK(after.rest.get() == before.rest.get());
  CHECK(after.meta.get() != before.meta.get());
  CHECK(*core.rv("Pod", "d", "a") == "5");
  CHECK(core.list_views(std::nullopt, {{"g", "y"}}).size() == 1);
  CHECK(core.list_views(std::nullopt, {}).at(0).view.phase == "Running");
  CHECK(core.peek("Pod", "d", "a")->rv == "5");
  CHECK(!core.peek("Pod", "d", "nope"));

  // remove while the history still references the sections
  const std::string expect = after.str();
  const size_t live_before = core.total_bytes();
  CHECK(core.remove("Pod", "d", "a", 6)->str() == expect);
  CHECK(!core.remove("Pod", "d", "a", 7));
  CHECK(core.total_bytes() < live_before);
  auto items = core.history_since(0, nullptr);
  CHECK(items.has_value());
  CHECK(items->size() == 4);  // ADDED, MODIFIED, MODIFIED, DELETED
  CHECK(items->back().event_type == "DELETED");
  CHECK(items->back().rv_override && *items->back().rv_override == 6);
  CHECK(items->back().blob.str() == expect);
  CHECK(!(*items)[0].rv_override);
  std::unordered_set<std::string> kinds{"Secret"};
  CHECK(core.history_since(0, &kinds)->empty());
  CHECK(core.history_since(5, nullptr)->size() == 1);

  // ring wrap: capacity 8, rvs 7..26 -> 19..26 retained
  for (int64_t rv = 7; rv <= 26; ++rv) {
    core.put("ConfigMap", "d", "c" + std::to_string(rv % 3),
             make_blob("\"kind\":\"ConfigMap\"", "{\"rv\":" + std::to_string(rv) + "}",
                       nullptr),
             make_fields(rv, "u-c", "x"), rv % 2 ? "ADDED" : "MODIFIED");
  }
  CHECK(core.history_size() == 8);
  CHECK(core.history_rvs().front() == 19);
  CHECK(!core.history_since(10, nullptr));         // oldest 19 > 10 + 1
  CHECK(!core.history_since(17, nullptr));         // 19 > 18
  CHECK(core.history_since(18, nullptr)->size() == 8);
  CHECK(core.history_since(26, nullptr)->empty());
  core.history_reset(30);
  CHECK(core.history_size() == 0);
  CHECK(!core.history_since(29, nullptr));         // below base
  CHECK(core.history_since(30, nullptr)->empty());
  core.history_reset(0, 4);
  for (int64_t rv = 31; rv <= 36; ++rv) {
    core.put("ConfigMap", "d", "c0",
             make_blob("\"kind\":\"ConfigMap\"", "{}", nullptr),
             make_fields(rv, "u-c", "x"), "MODIFIED");
  }
  CHECK(core.history_size() == 4);

  // index churn + owner index
  for (int i = 0; i < 200; ++i) {
    const std::string name = "p" + std::to_string(i % 10);
    core.put("Pod", "d", name,
             make_blob("\"kind\":\"Pod\"", "{}", "{}"),
             make_fields(100 + i, "u-" + name, i % 2 ? "x" : "y", "owner-1"),
             "MODIFIED");
    if (i % 7 == 0) core.remove("Pod", "d", name, 1000 + i);
  }
  const size_t pods = core.count("Pod");
  CHECK(core.dependents("owner-1").size() == pods);
  CHECK(core.list("Pod", std::nullopt, {{"g", "x"}}).size() +
            core.list("Pod", std::nullopt, {{"g", "y"}}).size() == pods);
  core.drop_owner("owner-1");
  CHECK(core.dependents("owner-1").empty());

  core.note_encode(true, 10);
  core.note_encode(false, 5);
  core.note_assembled(2, 40);
  core.note_fallback();
  const Stats s = core.stats();
  CHECK(s.full_encodes == 1 && s.partial_encodes == 1 && s.bytes_encoded == 15);
  CHECK(s.blobs_assembled == 2 && s.bytes_assembled == 40 && s.fallbacks == 1);
  CHECK(s.history_appends > 0);
}

// Writers allocate rvs and write under one lock, as the API server does;
// readers and removers run free. History rvs must come out strictly
// increasing, and every blob read must be one that some writer wrote whole.
static void multi_threaded() {
  StoreCore core(64);
  std::mutex server_lock;
  int64_t next_rv = 0;
  std::atomic<bool> stop{false};
  constexpr int kWriters = 6, kOps = 400, kKeys = 5;

  auto writer = [&](int id) {
    for (int i = 0; i < kOps; ++i) {
      const std::string name = "k" + std::to_string((id + i) % kKeys);
      std::lock_guard<std::mutex> g(server_lock);
      const int64_t rv = ++next_rv;
      const std::string tag = std::to_string(rv);
      switch (i % 4) {
        case 0:
        case 1:
          core.put("Pod", "d", name,
                   make_blob("\"kind\":\"Pod\",\"w\":" + tag, "{\"rv\":" + tag + "}",
                             ("{\"rv\":" + tag + "}").c_str()),
                   make_fields(rv, "u-" + name, id % 2 ? "x" : "y", "own"),
                   "MODIFIED");
          break;
        case 2: {
          Peek p;
          p.rv = tag;
          PodViewData view;
          view.name = name;
          if (!core.put_status("Pod", "d", name, sec("{\"rv\":" + tag + "}"),
                               sec("{\"rv\":" + tag + "}"), p, true, view,
                               "MODIFIED")) {
            --next_rv;  // nothing written, nothing recorded
          }
          break;
        }
        default:
          if (!core.remove("Pod", "d", name, rv)) --next_rv;
      }
    }
  };
  auto reader = [&]() {
    while (!stop.load()) {
      for (int k = 0; k < kKeys; ++k) {
        auto b = core.fetch("Pod", "d", "k" + std::to_string(k));
        if (b) {
          // meta and status are always written together
          CHECK(*b->meta == *b->status);
          CHECK(b->str().size() == b->size());
        }
      }
      auto items = core.history_since(0, nullptr);
      if (items) {
        for (const auto& it : *items) CHECK(it.blob.str().size() == it.blob.size());
      }
      std::vector<int64_t> rvs = core.history_rvs();
      for (size_t i = 1; i < rvs.size(); ++i) CHECK(rvs[i - 1] < rvs[i]);
      core.list("Pod", std::nullopt, {{"g", "x"}});
      core.list_views(std::nullopt, {});
      core.dependents("own");
      core.total_bytes();
      core.count("Pod");
    }
  };

  std::vector<std::thread> threads;
  for (int i = 0; i < kWriters; ++i) threads.emplace_back(writer, i);
  std::thread r1(reader), r2(reader);
  for (auto& t : threads) t.join();
  stop.store(true);
  r1.join();
  r2.join();

  std::vector<int64_t> rvs = core.history_rvs();
  CHECK(rvs.size() == 64);
  for (size_t i = 1; i < rvs.size(); ++i) CHECK(rvs[i - 1] < rvs[i]);
  CHECK(rvs.back() == next_rv);
  CHECK(core.dependents("own").size() == core.count("Pod"));
}

int main() {
  single_threaded();
  multi_threaded();
  std::puts("store_core_check OK");
  return 0;
}
