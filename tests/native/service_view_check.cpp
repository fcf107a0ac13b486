// Stand-alone driver for the Service views of
// kuberay_amd/_native/store_core.hpp (no Python). Built and run by
// tests/test_service_view_sanitizers.py under -fsanitize=address,undefined
// and again under -fsanitize=thread. Exits 0 when every check holds; prints
// the failed check and exits 1 otherwise.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
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

static Blob make_blob(const std::string& name) {
  Blob b;
  b.rest = sec("\"kind\":\"Service\",\"spec\":{}");
  b.meta = sec("{\"name\":\"" + name + "\"}");
  return b;
}

static ServicePortView port(const std::string& name, int64_t number,
                            bool has_node_port = false, int64_t node_port = 0) {
  ServicePortView p;
  p.name = name;
  p.port = number;
  p.has_port = true;
  p.has_node_port = has_node_port;
  p.node_port = node_port;
  return p;
}

static Fields service_fields(int64_t rv, const std::string& name,
                             const std::string& ip,
                             std::vector<ServicePortView> ports) {
  Fields f;
  f.rv = std::to_string(rv);
  f.uid = "u-" + name;
  f.has_service_view = true;
  f.service_view.name = name;
  f.service_view.ns = "d";
  f.service_view.cluster_ip = ip;
  f.service_view.ports = std::move(ports);
  return f;
}

static void single_threaded() {
  StoreCore core(8);

  // nothing stored, and a default Fields carries no view
  CHECK(!core.service_view("d", "svc"));
  Fields plain;
  plain.rv = "1";
  CHECK(!plain.has_service_view);
  core.put("Service", "d", "noview", make_blob("noview"), plain, "ADDED");
  CHECK(core.contains("Service", "d", "noview"));
  CHECK(!core.service_view("d", "noview"));

  // create
  core.put("Service", "d", "svc", make_blob("svc"),
           service_fields(2, "svc", "10.0.0.1",
                          {port("gcs", 6379), port("", 8265),
                           port("dash", 8265, true, 30265)}),
           "ADDED");
  std::optional<ServiceViewData> v = core.service_view("d", "svc");
  CHECK(v);
  CHECK(v->name == "svc" && v->ns == "d" && v->cluster_ip == "10.0.0.1");
  CHECK(v->ports.size() == 3);
  CHECK(v->ports[0].name == "gcs" && v->ports[0].port == 6379);
  CHECK(v->ports[0].has_port && !v->ports[0].has_node_port);
  CHECK(v->ports[1].name.empty());
  CHECK(v->ports[2].has_node_port && v->ports[2].node_port == 30265);
  // the view is per (namespace, name) and for Services only
  CHECK(!core.service_view("other", "svc"));
  core.put("Pod", "d", "svc", make_blob("svc"),
           service_fields(3, "svc", "1.1.1.1", {}), "ADDED");
  CHECK(core.service_view("d", "svc")->cluster_ip == "10.0.0.1");

  // a status write keeps the view
  Peek p;
  p.rv = "4";
  p.uid = "u-svc";
  CHECK(core.put_status("Service", "d", "svc", sec("{\"name\":\"svc\"}"),
                        sec("{\"loadBalancer\":{}}"), p, false, PodViewData{},
                        "MODIFIED"));
  v = core.service_view("d", "svc");
  CHECK(v && v->ports.size() == 3 && v->cluster_ip == "10.0.0.1");
  CHECK(*core.rv("Service", "d", "svc") == "4");

  // a spec update replaces it
  core.put("Service", "d", "svc", make_blob("svc"),
           service_fields(5, "svc", "None", {port("gcs", 6380)}), "MODIFIED");
  v = core.service_view("d", "svc");
  CHECK(v && v->cluster_ip == "None" && v->ports.size() == 1);
  CHECK(v->ports[0].port == 6380);

  // a full write without a view drops the old one
  Fields none;
  none.rv = "6";
  core.put("Service", "d", "svc", make_blob("svc"), none, "MODIFIED");
  CHECK(core.contains("Service", "d", "svc"));
  CHECK(!core.service_view("d", "svc"));

  // remove drops it; the history entry it leaves carries no view
  core.put("Service", "d", "svc", make_blob("svc"),
           service_fields(7, "svc", "", {}), "MODIFIED");
  v = core.service_view("d", "svc");
  CHECK(v && v->cluster_ip.empty() && v->ports.empty());
  CHECK(core.remove("Service", "d", "svc", 8));
  CHECK(!core.service_view("d", "svc"));
  CHECK(!core.contains("Service", "d", "svc"));

  // a copy handed out stays valid after the entry is gone
  core.put("Service", "d", "gone", make_blob("gone"),
           service_fields(9, "gone", "10.0.0.9", {port("a", 1), port("b", 2)}),
           "ADDED");
  std::optional<ServiceViewData> kept = core.service_view("d", "gone");
  core.remove("Service", "d", "gone");
  CHECK(kept && kept->ports.size() == 2 && kept->ports[1].name == "b");
}

static void multi_threaded() {
  StoreCore core(64);
  constexpr int kWriters = 3, kReaders = 3, kRounds = 400;
  std::atomic<bool> stop{false};
  std::atomic<int> bad{0};
  std::vector<std::thread> threads;
  for (int w = 0; w < kWriters; ++w) {
    threads.emplace_back([&core, w] {
      const std::string name = "svc-" + std::to_string(w);
      for (int i = 0; i < kRounds; ++i) {
        // every port of a view written in round i carries the number i
        std::vector<ServicePortView> ports;
        for (int k = 0; k < 1 + i % 4; ++k) ports.push_back(port("p", i));
        core.put("Service", "d", name, make_blob(name),
                 service_fields(i, name, std::to_string(i), std::move(ports)),
                 "MODIFIED");
        Peek p;
        p.rv = std::to_string(i);
        core.put_status("Service", "d", name, sec("{}"), sec("{}"), p, false,
                        PodViewData{}, "MODIFIED");
        if (i % 7 == 0) core.remove("Service", "d", name, i);
      }
    });
  }
  for (int r = 0; r < kReaders; ++r) {
    threads.emplace_back([&core, &stop, &bad, r] {
      const std::string name = "svc-" + std::to_string(r % kWriters);
      while (!stop.load()) {
        std::optional<ServiceViewData> v = core.service_view("d", name);
        if (!v) continue;
        // a view is read whole: one round's clusterIP with that round's ports
        for (const ServicePortView& p : v->ports) {
          if (std::to_string(p.port) != v->cluster_ip) bad.fetch_add(1);
        }
        if (v->name != name) bad.fetch_add(1);
      }
    });
  }
  for (int w = 0; w < kWriters; ++w) threads[w].join();
  stop.store(true);
  for (size_t t = kWriters; t < threads.size(); ++t) threads[t].join();
  CHECK(bad.load() == 0);
}

int main() {
  single_threaded();
  multi_threaded();
  std::printf("service_view_check OK\n");
  return 0;
}
