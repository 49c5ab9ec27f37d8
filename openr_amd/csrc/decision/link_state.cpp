// link_state.cpp — LinkState mirror (see link_state.h); SPF on the engine.
#include "link_state.h"
#include "../common/knobs.h"

#include <cstdlib>
#include <cstring>
#include <numeric>
#include <set>
#include <algorithm>
#include <unordered_set>
#include <system_error>
#include <thread>
#include <functional>
#include <map>
#include <stdexcept>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <cstdio>
#include <thread>
#include <tuple>

namespace odl {

namespace {

// folly::hash::hash_128_to_64 (folly rev 04c2275157a3e44c1d1fa1df75835fe4ec8a7b1e,
// folly/hash/Hash.h), used by folly's std::hash<std::pair> specialisation that
// the reference's Link hash relies on (LinkState.cpp:134-138).
inline uint64_t fold(uint64_t hi, uint64_t lo) {
  constexpr uint64_t kMul = 0x9ddfea08eb382d69ULL;
  uint64_t a = (lo ^ hi) * kMul;
  a ^= a >> 47;
  uint64_t b = (hi ^ a) * kMul;
  b ^= b >> 47;
  return b * kMul;
}

inline uint64_t hashEnd(const std::string& node, const std::string& iface) {
  const std::hash<std::string> h;
  return fold(h(node), h(iface));  // std::hash<std::pair<string, string>>
}

constexpr uint32_t kInf = OSPF_DIST_INF;

}  // namespace

// ---------------------------------------------------------------- Link
// One thread per LinkState frees dropped memos, in the order they were
// dropped; the LinkState's destructor drains the queue and joins it, so no
// release outlives the object (r04 had a detached thread per event). Only
// memory unreachable from the LinkState is handed over: the SpfResults own
// their rows and entries, and the Links / snapshots they share are
// reference-counted (std::shared_ptr, atomic counts).
struct MemoReaper {
  using Memo = std::unordered_map<std::string, SpfResult>;
  struct Dead {
    Memo a, b;
    std::unordered_map<std::string, std::vector<Path>> k;
  };
  std::mutex mu;
  std::condition_variable cv;
  std::deque<std::unique_ptr<Dead>> q;
  bool stop = false;
  std::thread th;
  MemoReaper() : th([this] { loop(); }) {}
  ~MemoReaper() {
    {
      std::lock_guard<std::mutex> g(mu);
      stop = true;
    }
    cv.notify_one();
    th.join();
  }
  void push(std::unique_ptr<Dead> d) {
    {
      std::lock_guard<std::mutex> g(mu);
      q.push_back(std::move(d));
    }
    cv.notify_one();
  }
  void loop() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [this] { return stop || !q.empty(); });
      if (q.empty()) return;  // stop, and everything freed
      std::unique_ptr<Dead> d = std::move(q.front());
      q.pop_front();
      lk.unlock();
      d.reset();
      lk.lock();
    }
  }
};

size_t Link::hashOf(const End& lo, const End& hi) {
  return fold(hashEnd(lo.node, lo.iface), hashEnd(hi.node, hi.iface));
}

size_t LinkState::AdjKeyHash::operator()(const AdjKey& k) const {
  const std::hash<std::string_view> h;
  return fold(h(k.other), fold(h(k.ifn), h(k.oifn)));
}

static bool endLess(const std::string& n1, const std::string& i1, const std::string& n2,
                    const std::string& i2) {
  const int c = n1.compare(n2);
  return c < 0 || (c == 0 && i1 < i2);
}

// The ends are stored once, end_[lo_] holding the smaller (node, iface) pair
// -- the reference's n1/if1 after its ordering (LinkState.cpp:95-110).
Link::Link(const std::string& n1, const Adjacency& a1, const std::string& n2, const Adjacency& a2)
    : hash([&] {
        return endLess(n2, a2.ifName, n1, a1.ifName)
                   ? fold(hashEnd(n2, a2.ifName), hashEnd(n1, a1.ifName))
                   : fold(hashEnd(n1, a1.ifName), hashEnd(n2, a2.ifName));
      }()) {
  lo_ = endLess(n2, a2.ifName, n1, a1.ifName) ? 1 : 0;
  const Adjacency* adj[2] = {&a1, &a2};
  const std::string* nn[2] = {&n1, &n2};
  for (int i = 0; i < 2; ++i) {
    end_[i].node = *nn[i];
    end_[i].iface = adj[i]->ifName;
    end_[i].metric = (Metric)(int64_t)adj[i]->metric;  // i32 -> u64 as the reference
    end_[i].overload = (bool)adj[i]->isOverloaded;
    end_[i].adjLabel = adj[i]->adjLabel;
    end_[i].weight = adj[i]->weight;
  }
}

Link::End& Link::endOf(const std::string& n) {
  if (end_[0].node == n) return end_[0];
  if (end_[1].node == n) return end_[1];
  throw std::invalid_argument(n);
}
const Link::End& Link::endOf(const std::string& n) const {
  return const_cast<Link*>(this)->endOf(n);
}
const std::string& Link::otherNode(const std::string& n) const {
  if (end_[0].node == n) return end_[1].node;
  if (end_[1].node == n) return end_[0].node;
  throw std::invalid_argument(n);
}
const std::string& Link::ifaceFrom(const std::string& n) const { return endOf(n).iface; }
Metric Link::metricFrom(const std::string& n) const { return endOf(n).metric.value(); }
bool Link::overloadFrom(const std::string& n) const { return endOf(n).overload.value(); }
int32_t Link::adjLabelFrom(const std::string& n) const { return endOf(n).adjLabel; }
int64_t Link::weightFrom(const std::string& n) const { return endOf(n).weight; }

bool Link::setMetricFrom(const std::string& n, Metric m, Metric holdUpTtl, Metric holdDownTtl) {
  return endOf(n).metric.updateValue(m, holdUpTtl, holdDownTtl);
}
bool Link::setOverloadFrom(const std::string& n, bool ov, Metric holdUpTtl, Metric holdDownTtl) {
  const bool wasUp = isUp();
  endOf(n).overload.updateValue(ov, holdUpTtl, holdDownTtl);
  return wasUp != isUp();
}
bool Link::decrementHolds() {
  bool expired = false;
  if (holdUpTtl_ != 0) expired |= --holdUpTtl_ == 0;
  for (End& e : end_) {
    expired |= e.metric.decrementTtl();
    expired |= e.overload.decrementTtl();
  }
  return expired;
}
bool Link::hasHolds() const {
  return holdUpTtl_ != 0 || end_[0].metric.hasHold() || end_[1].metric.hasHold() ||
         end_[0].overload.hasHold() || end_[1].overload.hasHold();
}
void Link::setAdjLabelFrom(const std::string& n, int32_t l) { endOf(n).adjLabel = l; }
void Link::setWeightFrom(const std::string& n, int64_t w) { endOf(n).weight = w; }

bool Link::sameLink(const Link& o) const {
  const End &a = end_[lo_], &b = end_[lo_ ^ 1], &c = o.end_[o.lo_], &d = o.end_[o.lo_ ^ 1];
  return hash == o.hash && a.node == c.node && a.iface == c.iface && b.node == d.node &&
         b.iface == d.iface;
}
bool Link::orderedBefore(const Link& o) const {
  if (hash != o.hash) return hash < o.hash;
  const End &a = end_[lo_], &b = end_[lo_ ^ 1], &c = o.end_[o.lo_], &d = o.end_[o.lo_ ^ 1];
  return std::tie(a.node, a.iface, b.node, b.iface) < std::tie(c.node, c.iface, d.node, d.iface);
}
std::string Link::key() const {
  const End &a = end_[lo_], &b = end_[lo_ ^ 1];
  return a.node + "%" + a.iface + "|" + b.node + "%" + b.iface;
}

// ---------------------------------------------------------------- LinkState
LinkState::LinkState(std::string area, int device)
    : area_(std::move(area)), device_(device), devices_{device} {
  hostOnly_ = knob_flag(Knob::ODL_HOST_SPF);
  degradeOnError_ = !knob_flag(Knob::ODL_STRICT_ENGINE);
}

LinkState::LinkState(std::string area, std::vector<int> devices)
    : area_(std::move(area)), device_(devices.empty() ? 0 : devices[0]), devices_(std::move(devices)) {
  if (devices_.empty()) throw std::invalid_argument("LinkState: no device");
  hostOnly_ = knob_flag(Knob::ODL_HOST_SPF);
  degradeOnError_ = !knob_flag(Knob::ODL_STRICT_ENGINE);
}

LinkState::~LinkState() {
  joinOpen();
  reaper_.reset();  // drains the dropped memos, joins the thread
  trackDropDev();
  dropSweep();
  if (multi_) ospf_multi_close(multi_);
  else if (engine_) ospf_close(engine_);
}

const LinkSet& LinkState::linksFromNode(const std::string& node) const {
  static const LinkSet kEmpty;
  auto it = linkMap_.find(node);
  return it == linkMap_.end() ? kEmpty : it->second;
}

bool LinkState::isNodeOverloaded(const std::string& node) const {
  auto it = nodeOverloads_.find(node);
  return it != nodeOverloads_.end() && it->second.value();
}

LinkStateChange LinkState::decrementHolds() {
  LinkStateChange ch;
  for (auto& shard : allLinks_)
    for (const auto& l : shard) ch.topologyChanged |= l->decrementHolds();
  for (auto& kv : nodeOverloads_) ch.topologyChanged |= kv.second.decrementTtl();
  // an expired hold changes what the snapshot holds (metrics, up state, node
  // overload): the memo is dropped (LinkState.cpp:530-533) and the CSR taken
  // again
  if (ch.topologyChanged) invalidate();
  return ch;
}

bool LinkState::hasHolds() const {
  for (const auto& shard : allLinks_)
    for (const auto& l : shard)
      if (l->hasHolds()) return true;
  for (const auto& kv : nodeOverloads_)
    if (kv.second.hasHold()) return true;
  return false;
}

LinkPtr LinkState::makeLink(const std::string& node, const Adjacency& adj) const {
  auto other = adjDbs_.find(adj.otherNodeName);
  if (other == adjDbs_.end()) return nullptr;
  auto idx = adjIndex_.find(adj.otherNodeName);
  if (idx == adjIndex_.end()) return nullptr;
  auto hit = idx->second.find(AdjKey{node, adj.otherIfName, adj.ifName});
  if (hit == idx->second.end()) return nullptr;
  return std::make_shared<Link>(node, adj, adj.otherNodeName,
                                other->second.adjacencies[hit->second]);
}

void LinkState::addLink(const LinkPtr& l) {
  if (!linkMap_[l->lowNode()].insert(l).second || !linkMap_[l->highNode()].insert(l).second ||
      !shardOf(*l).insert(l).second)
    throw std::logic_error("duplicate link " + l->key());
}

void LinkState::removeLink(const LinkPtr& l) {
  if (!linkMap_.at(l->lowNode()).erase(l) || !linkMap_.at(l->highNode()).erase(l) ||
      !shardOf(*l).erase(l))
    throw std::logic_error("missing link " + l->key());
}

std::vector<LinkPtr> LinkState::sortedLinksOf(const std::string& node) const {
  const LinkSet& s = linksFromNode(node);
  std::vector<LinkPtr> v(s.begin(), s.end());
  std::sort(v.begin(), v.end(), [](const LinkPtr& a, const LinkPtr& b) {
    return a->orderedBefore(*b);
  });
  return v;
}

static size_t V_of(const LinkState::Csr& c) { return c.names.size(); }

void LinkState::clearMemo() {
  if (memoMetric_.empty() && memoHops_.empty() && memoKsp_.empty()) return;
  // A route build materialises every entry of its results (~100k node
  // results with next-hop sets and path links at F100k): freeing them took
  // most of an event's apply time, so the reaper thread frees them.
  auto dead = std::make_unique<MemoReaper::Dead>();
  dead->a.swap(memoMetric_);
  dead->b.swap(memoHops_);
  dead->k.swap(memoKsp_);
  if (!reaper_) {
    try {
      reaper_ = std::make_unique<MemoReaper>();
    } catch (const std::system_error&) {  // no thread to spare: free here
      return;
    }
  }
  reaper_->push(std::move(dead));
}

void LinkState::invalidate() {
  ++version_;
  dropSweep();
  clearMemo();
}

LinkStateChange LinkState::updateAdjacencyDatabase(const AdjacencyDatabase& db, Metric holdUpTtl,
                                                   Metric holdDownTtl) {
  LinkStateChange ch;
  const std::string me = db.thisNodeName;
  const bool known = adjDbs_.count(me) > 0;
  const int32_t priorLabel = known ? adjDbs_.at(me).nodeLabel : 0;
  bool structural = !known;  // a link or node added / removed (incremental mode)
  std::vector<LinkDelta> deltas;
  std::vector<std::string> nodeDeltas;
  std::vector<LinkPtr> removedLinks;
  auto& idx = adjIndex_[me];
  idx.clear();  // (its views point into the database replaced here)
  const AdjacencyDatabase& kept = adjDbs_[me] = db;
  for (uint32_t i = 0; i < kept.adjacencies.size(); ++i) {
    const auto& a = kept.adjacencies[i];
    idx.emplace(AdjKey{a.otherNodeName, a.ifName, a.otherIfName}, i);
  }

  std::vector<LinkPtr> before = sortedLinksOf(me);
  std::vector<LinkPtr> after;
  after.reserve(db.adjacencies.size());
  for (const auto& a : db.adjacencies)
    if (LinkPtr l = makeLink(me, a)) after.push_back(std::move(l));
  std::sort(after.begin(), after.end(),
            [](const LinkPtr& a, const LinkPtr& b) { return a->orderedBefore(*b); });

  auto ov = nodeOverloads_.find(me);
  if (ov == nodeOverloads_.end()) {
    nodeOverloads_.emplace(me, db.isOverloaded);  // a new node is not a change
  } else {
    const bool was = ov->second.value();
    ch.topologyChanged |= ov->second.updateValue(db.isOverloaded, holdUpTtl, holdDownTtl);
    if (ov->second.value() != was) nodeDeltas.push_back(me);
  }
  ch.nodeLabelChanged = priorLabel != db.nodeLabel;

  // two-pointer merge of old vs new link sets (both in Link::operator< order)
  size_t i = 0, j = 0;
  while (i < after.size() || j < before.size()) {
    const bool takeNew = i < after.size() && (j == before.size() || after[i]->orderedBefore(*before[j]));
    const bool takeOld = !takeNew && j < before.size() &&
                         (i == after.size() || before[j]->orderedBefore(*after[i]));
    if (takeNew) {
      structural = true;
      after[i]->setHoldUpTtl(holdUpTtl);
      ch.topologyChanged |= after[i]->isUp();
      addLink(after[i]);
      ch.addedLinks.push_back(after[i]);
      ++i;
    } else if (takeOld) {
      structural = true;
      ch.topologyChanged |= before[j]->isUp();
      removeLink(before[j]);
      removedLinks.push_back(before[j]);
      ++j;
    } else {
      const Link& fresh = *after[i];
      Link& kept = *before[j];
      if (fresh.metricFrom(me) != kept.metricFrom(me) ||
          fresh.overloadFrom(me) != kept.overloadFrom(me))
        deltas.push_back(LinkDelta{before[j], kept.isUp(), kept.metricFrom(kept.lowNode()),
                                   kept.metricFrom(kept.highNode())});
      if (fresh.metricFrom(me) != kept.metricFrom(me))
        ch.topologyChanged |= kept.setMetricFrom(me, fresh.metricFrom(me), holdUpTtl, holdDownTtl);
      if (fresh.overloadFrom(me) != kept.overloadFrom(me))
        ch.topologyChanged |=
            kept.setOverloadFrom(me, fresh.overloadFrom(me), holdUpTtl, holdDownTtl);
      if (fresh.adjLabelFrom(me) != kept.adjLabelFrom(me)) {
        kept.setAdjLabelFrom(me, fresh.adjLabelFrom(me));
        ch.linkAttributesChanged = true;
      }
      if (fresh.weightFrom(me) != kept.weightFrom(me)) {
        kept.setWeightFrom(me, fresh.weightFrom(me));
        ch.linkAttributesChanged = true;
      }
      ++i;
      ++j;
    }
  }
  // Incremental mode: same nodes and links, CSR current -> patch in place
  // (not in host-metric mode, and only while the patched metrics keep the
  // engine contract: an in-range increase raises the distance bound by at
  // most the new metric)
  bool keepsContract = !hostMetric_;
  uint64_t bound = distBound_;
  for (const auto& d : deltas) {
    for (const Metric m : {d.link->metricFrom(d.link->lowNode()), d.link->metricFrom(d.link->highNode())}) {
      keepsContract &= m >= 1 && m <= 0xFFFFFFFFull;
      bound += keepsContract ? m : 0;
    }
  }
  // links added between known nodes: their metrics join the bound
  for (const auto& l : ch.addedLinks)
    for (const Metric m : {l->metricFrom(l->lowNode()), l->metricFrom(l->highNode())}) {
      keepsContract &= m >= 1 && m <= 0xFFFFFFFFull;
      bound += keepsContract ? m : 0;
    }
  keepsContract &= bound < 0xFFFFFFFFull;
  // [LINK UP] / [LINK DOWN] between known nodes (LinkState.cpp:632-657): the
  // snapshot and the device graph are patched in place; the memo is dropped on
  // a topology change as in the reference (:751-754) -- in incremental mode
  // too (its kept-root rule covers metric / up / overload changes only)
  if (known && structural && snapVersion_ == version_ && keepsContract &&
      !knob_flag(Knob::ODL_NO_LINK_PATCH)) {
    if (ch.topologyChanged || incremental_) {
      if (incremental_) incStats_.dropped += memoMetric_.size() + memoHops_.size();
      clearMemo();
    }
    // kept links' metric / up changes first (on the rows as they are), so the
    // rebuilt rows and their partners agree when the structure is patched
    if (!deltas.empty() || !nodeDeltas.empty()) patchGraph(deltas, nodeDeltas);
    patchStructure(ch.addedLinks, removedLinks);
    return ch;
  }
  if (incremental_ && !structural && snapVersion_ == version_ && keepsContract) {
    distBound_ = bound;
    if (ch.topologyChanged) applyIncremental(deltas, nodeDeltas);
    return ch;
  }
  // The same nodes and links: the snapshot stays (node ids are name ranks,
  // unchanged). Metric / up / overload changes are patched into the CSR and
  // the device graph in place; the memo is dropped on a topology change,
  // exactly as in the reference (LinkState.cpp:751-754), and survives
  // attribute-only updates (:721-724: labels, weights).
  if (!structural && snapVersion_ == version_ && keepsContract) {
    distBound_ = bound;
    if (ch.topologyChanged) clearMemo();
    if (!deltas.empty() || !nodeDeltas.empty()) patchGraph(deltas, nodeDeltas);
    return ch;
  }
  // a node added while the snapshot is current: its (empty) row enters in
  // place, then the links it formed (peers that already advertised it)
  // patch their rows; the device graph reloads on its next use
  if (!known && snapVersion_ == version_ && keepsContract && !knob_flag(Knob::ODL_NO_LINK_PATCH)) {
    if (ch.topologyChanged) clearMemo();
    engineVersion_ = 0;
    const auto& nm = csr_->names;
    const uint32_t k = (uint32_t)(std::lower_bound(nm.begin(), nm.end(), me) - nm.begin());
    csrInsertNode(k, me, db.isOverloaded);
    patchStructure(ch.addedLinks, {});
    return ch;
  }
  // a metric leaving the engine contract, or a change without a current
  // snapshot: the CSR is snapshotted again
  if (ch.topologyChanged) {
    invalidate();
  } else {
    ++version_;
  }
  return ch;
}

// Bulk path: every database is a node not yet known. Such a node has no
// links before its own update (a link needs both databases), and its update
// creates the links to the nodes known by then -- before the batch, earlier
// in it, or itself -- in Link order, inserted into the low then the high
// node's LinkSet and into allLinks_. Built here: databases and adjacency
// indexes per node in parallel, each node's created links in parallel (the
// indexes are only read), then every node's LinkSet filled in parallel with
// its links in the sequential insertion order (creation order), so each
// unordered_set ends up with the same buckets and iteration order.
std::vector<LinkStateChange> LinkState::updateAdjacencyDatabases(std::vector<AdjacencyDatabase>& dbs,
                                                                Metric holdUpTtl,
                                                                Metric holdDownTtl) {
  const auto tIn = std::chrono::steady_clock::now();
  const uint32_t n = (uint32_t)dbs.size();
  std::vector<LinkStateChange> out(n);
  // (the bulk path makes links without holds)
  bool bulk = n >= 64 && holdUpTtl == 0 && !knob_flag(Knob::ODL_NO_BULK_INGEST);
  std::unordered_map<std::string, uint32_t> posOf;
  if (bulk) {
    posOf.reserve(n);
    for (uint32_t i = 0; i < n && bulk; ++i)
      bulk = !adjDbs_.count(dbs[i].thisNodeName) && posOf.emplace(dbs[i].thisNodeName, i).second;
  }
  if (!bulk) {
    for (uint32_t i = 0; i < n; ++i) out[i] = updateAdjacencyDatabase(dbs[i], holdUpTtl, holdDownTtl);
    return out;
  }

  using Clock = std::chrono::steady_clock;
  const bool timing = knob_flag(Knob::ODL_SPF_TIMING);
  Clock::time_point tp[6];
  tp[0] = Clock::now();
  std::vector<AdjacencyDatabase*> dbp(n);
  std::vector<std::unordered_map<AdjKey, uint32_t, AdjKeyHash>*> idxp(n);
  // (no order of these maps or of allLinks_ is observed: node ids are name
  // ranks; only the per-node LinkSets' iteration order is, and those are not
  // reserved)
  adjDbs_.reserve(adjDbs_.size() + n);
  adjIndex_.reserve(adjIndex_.size() + n);
  nodeOverloads_.reserve(nodeOverloads_.size() + n);
  linkMap_.reserve(linkMap_.size() + n);
  for (uint32_t i = 0; i < n; ++i) {
    const std::string me = dbs[i].thisNodeName;
    nodeOverloads_.emplace(me, dbs[i].isOverloaded);  // a new node is not a change
    out[i].nodeLabelChanged = dbs[i].nodeLabel != 0;
    AdjacencyDatabase& slot = adjDbs_[me];
    slot = std::move(dbs[i]);
    dbp[i] = &slot;
    idxp[i] = &adjIndex_[me];
  }
  parallelFor(n, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t i = lo; i < hi; ++i) {
      auto& idx = *idxp[i];
      idx.clear();
      const auto& adj = dbp[i]->adjacencies;
      idx.reserve(adj.size());
      for (uint32_t k = 0; k < adj.size(); ++k)
        idx.emplace(AdjKey{adj[k].otherNodeName, adj[k].ifName, adj[k].otherIfName}, k);
    }
  }, 256);
  // links each update creates, in Link order
  tp[1] = Clock::now();
  // (link, batch position of its other end or kNone) per update
  std::vector<std::vector<std::pair<LinkPtr, uint32_t>>> created(n);
  parallelFor(n, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t i = lo; i < hi; ++i) {
      const AdjacencyDatabase& db = *dbp[i];
      auto& v = created[i];
      for (const auto& a : db.adjacencies) {
        auto p = posOf.find(a.otherNodeName);
        if (p != posOf.end() && p->second > i) continue;  // created by that node's update
        if (LinkPtr l = makeLink(db.thisNodeName, a))
          v.emplace_back(std::move(l), p != posOf.end() ? p->second : kInf);
      }
      std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) {
        return a.first->orderedBefore(*b.first);
      });
    }
  }, 256);
  tp[2] = Clock::now();
  // every touched node's insertions in creation order (low end, then high)
  std::unordered_map<std::string, uint32_t> other;  // nodes known before the batch
  // (pointers into out[i].addedLinks, reserved up front: no reallocation)
  std::vector<std::vector<const LinkPtr*>> ins(n);
  std::array<std::vector<const LinkPtr*>, kLinkShards> shardIns;
  bool anyTopo = false;
  for (uint32_t i = 0; i < n; ++i) {
    out[i].addedLinks.reserve(created[i].size());
    for (auto& c : created[i]) {
      out[i].addedLinks.push_back(std::move(c.first));
      const LinkPtr* l = &out[i].addedLinks.back();
      if (c.second == i) throw std::logic_error("duplicate link " + (*l)->key());  // a self-link
      uint32_t o = c.second;
      if (o == kInf) {
        auto q = other.emplace((*l)->otherNode(dbp[i]->thisNodeName), (uint32_t)ins.size());
        if (q.second) ins.emplace_back();
        o = q.first->second;
      }
      const bool meLow = (*l)->lowNode() == dbp[i]->thisNodeName;
      ins[meLow ? i : o].push_back(l);
      ins[meLow ? o : i].push_back(l);
      out[i].topologyChanged |= (*l)->isUp();
      shardIns[((*l)->hash >> 7) % kLinkShards].push_back(l);
    }
    anyTopo |= out[i].topologyChanged;
  }
  created = {};
  tp[3] = Clock::now();
  std::vector<LinkSet*> setp(ins.size());
  for (uint32_t i = 0; i < n; ++i) setp[i] = &linkMap_[dbp[i]->thisNodeName];
  for (const auto& o : other) setp[o.second] = &linkMap_[o.first];
  std::atomic<bool> dup{false};
  parallelFor((uint32_t)ins.size(), [&](uint32_t lo, uint32_t hi) {
    for (uint32_t u = lo; u < hi; ++u)
      for (const LinkPtr* l : ins[u])
        if (!setp[u]->insert(*l).second) dup = true;
  }, 256);
  parallelFor(kLinkShards, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t s = lo; s < hi; ++s) {
      allLinks_[s].reserve(allLinks_[s].size() + shardIns[s].size());
      for (const LinkPtr* l : shardIns[s])
        if (!allLinks_[s].insert(*l).second) dup = true;
    }
  }, 1);
  tp[4] = Clock::now();
  if (timing) {
    auto ms = [&](int a) { return std::chrono::duration<double, std::milli>(tp[a + 1] - tp[a]).count(); };
    std::fprintf(stderr, "ODL_INGEST dbs=%u check_ms=%.1f index_ms=%.1f links_ms=%.1f order_ms=%.1f sets_ms=%.1f\n",
                 n, std::chrono::duration<double, std::milli>(tp[0] - tIn).count(), ms(0), ms(1), ms(2), ms(3));
  }
  if (dup) throw std::logic_error("duplicate link in an adjacency database batch");
  // one version step per database, as in turn (a new node is structural)
  version_ += n - (anyTopo ? 1u : 0u);
  if (anyTopo) invalidate();
  // (after the ingest, not beside it: the HIP runtime's start beside the
  // ingest's page-fault-heavy host work slowed the ingest by ~150-290 ms
  // at F100k, more than it saved the first getSpfResult, c9 vs c5)
  startOpen(adjDbs_.size());
  return out;
}

LinkStateChange LinkState::deleteAdjacencyDatabase(const std::string& node) {
  LinkStateChange ch;
  auto db = adjDbs_.find(node);
  if (db == adjDbs_.end()) return ch;
  // in place when the snapshot is current: the node's links leave their
  // rows (patchStructure), then its empty row leaves (ids above it move)
  const bool inPlace = snapVersion_ == version_ && !hostMetric_ && csr_->ids.count(node) &&
                       !knob_flag(Knob::ODL_NO_LINK_PATCH);
  std::vector<LinkPtr> removed;
  auto lm = linkMap_.find(node);
  if (lm != linkMap_.end()) {
    for (const auto& l : lm->second) {
      if (!linkMap_.at(l->otherNode(node)).erase(l) || !shardOf(*l).erase(l))
        throw std::logic_error("inconsistent link map");
      removed.push_back(l);
    }
    linkMap_.erase(lm);
    nodeOverloads_.erase(node);
  }
  adjDbs_.erase(db);
  adjIndex_.erase(node);
  ch.topologyChanged = true;
  if (!inPlace) {
    invalidate();
    return ch;
  }
  clearMemo();  // LinkState.cpp:751-754
  engineVersion_ = 0;  // the node count changes: the device graph reloads
  const uint32_t k = csr_->ids.at(node);
  patchStructure({}, removed);
  csrEraseNode(k);
  ++version_;
  snapVersion_ = version_;
  return ch;
}

// ---------------------------------------------------------------- snapshot

// Rows in parallel (threads over node ranges; the link sets are only read):
// 1. each row gathers its links (neighbour id, linksFromNode position, metric
//    from this end) and counts the links it sees first (smaller end id),
//    recording its own id on its end of each Link;
// 2. prefix sums give row offsets and link ids -- the same ids a sequential
//    sweep in (node id, linksFromNode order) hands out on first sight;
// 3. the lower end writes the link id into the Link, the upper end reads it;
// 4. rows are sorted by (neighbour id, rank) and written, then twins.
const LinkState::Csr& LinkState::snapshot() {
  if (snapVersion_ == version_) return *csr_;
  const bool tm = knob_flag(Knob::ODL_SNAP_TIMING);
  auto t0 = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!tm) return;
    auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "snapshot %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(t - t0).count());
    t0 = t;
  };
  ++topoStats_.snapshots;
  Csr c;
  {
    // sorted by (first 8 bytes big-endian, then the whole name): 16-B keys
    // move and compare as integers (the string sort's merges had moved and
    // compared strings); the order is the names' byte-wise order either way
    struct NameKey {
      uint64_t k;
      const std::string* s;
      bool operator<(const NameKey& o) const { return k != o.k ? k < o.k : *s < *o.s; }
    };
    // the map's buckets walked on threads (its nodes are scattered on the
    // heap: a serial walk was ~14 ms of cache misses at 100k nodes)
    constexpr uint32_t kParts = 64;
    const size_t nbk = adjDbs_.bucket_count();
    std::vector<std::vector<NameKey>> part(kParts);
    parallelFor(kParts, [&](uint32_t lo, uint32_t hi) {
      for (uint32_t p = lo; p < hi; ++p) {
        auto& out = part[p];
        for (size_t b = nbk * p / kParts; b < nbk * (p + 1) / kParts; ++b)
          for (auto it = adjDbs_.begin(b); it != adjDbs_.end(b); ++it) {
            const std::string& n = it->first;
            uint64_t k = 0;
            for (size_t i = 0; i < std::min<size_t>(8, n.size()); ++i)
              k |= (uint64_t)(uint8_t)n[i] << (56 - 8 * i);
            out.push_back({k, &n});
          }
      }
    }, 1);
    std::vector<NameKey> keyed;
    keyed.reserve(adjDbs_.size());
    for (auto& v : part) keyed.insert(keyed.end(), v.begin(), v.end());
    parallelSort(keyed);
    c.names.reserve(keyed.size());
    for (const auto& x : keyed) c.names.push_back(*x.s);
  }
  lap("names sorted");
  c.ids.reserve(c.names.size() * 2);
  for (uint32_t i = 0; i < c.names.size(); ++i) c.ids.emplace(c.names[i], i);
  lap("names");
  const uint32_t V = (uint32_t)c.names.size();
  c.rowPtr.assign(V + 1, 0);
  c.noTransit.assign(V, 0);
  struct Ent {
    uint32_t v, rank, metric;
    uint8_t up, low, end;
    const LinkPtr* link;
  };
  std::vector<std::vector<Ent>> rows(V);
  std::vector<uint32_t> nfirst(V + 1, 0);
  std::vector<uint8_t> rowBad(V, 0);
  std::vector<uint64_t> rowMax(V, 0);
  parallelFor(V, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t u = lo; u < hi; ++u) {
      const std::string& un = c.names[u];
      c.noTransit[u] = isNodeOverloaded(un) ? 1 : 0;
      const LinkSet& ls = linksFromNode(un);
      auto& row = rows[u];
      row.reserve(ls.size());
      uint32_t rank = 0, nf = 0;
      for (const auto& l : ls) {
        Ent e;
        e.end = (uint8_t)l->endIndex(un);
        l->snapEnd[e.end] = u;
        if (e.end == 0 && l->selfLoop()) l->snapEnd[1] = u;
        const Metric m = l->metricOfEnd(e.end);
        e.v = kInf;  // the other end's id: written by its own row
        e.rank = rank++;
        // a metric outside [1, 2^32) (0, or a negative i32 wrapped to u64) is
        // outside the engine contract: the snapshot goes to host mode and the
        // engine (hop-count runs only) sees 1
        const bool inRange = m >= 1 && m <= 0xFFFFFFFFull;
        e.metric = inRange ? (uint32_t)m : 1u;
        if (!inRange) rowBad[u] = 1;
        rowMax[u] = std::max<uint64_t>(rowMax[u], inRange ? m : 0);
        e.up = l->isUp() ? 1 : 0;
        // the lower end by name = by id sees the link first in id order
        e.low = (e.end == l->lowIndex() || l->selfLoop()) ? 1 : 0;
        e.link = &l;
        nf += e.low;
        row.push_back(e);
      }
      nfirst[u + 1] = nf;
      c.rowPtr[u + 1] = (uint32_t)row.size();
    }
  });
  for (uint32_t u = 0; u < V; ++u) {
    nfirst[u + 1] += nfirst[u];
    c.rowPtr[u + 1] += c.rowPtr[u];
  }
  // A simple path leaves each node at most once, so sum_u max_out(u) bounds
  // every shortest distance: below 2^32 - 1 (the engine's unreached value)
  // the engine's u32 distances cannot overflow.
  uint64_t bound = 0;
  bool bad = false;
  for (uint32_t u = 0; u < V; ++u) {
    bad |= rowBad[u] != 0;
    bound = std::min<uint64_t>(bound + rowMax[u], ~0ull >> 1);
  }
  distBound_ = bound;
  hostMetric_ = bad || bound >= 0xFFFFFFFFull;
  lap("gather");
  const size_t E = c.rowPtr[V];
  c.links.resize(nfirst[V]);
  parallelFor(V, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t u = lo; u < hi; ++u) {
      uint32_t lid = nfirst[u];
      for (auto& e : rows[u]) {
        e.v = (*e.link)->snapEnd[e.end ^ 1];
        if (!e.low) continue;
        (*e.link)->snapLid = lid;
        c.links[lid++] = *e.link;
      }
    }
  });
  lap("link ids");
  // room for the links patchStructure may add in place
  for (auto* v : {&c.col, &c.metric, &c.linkId, &c.twin, &c.linkRank}) v->reserve(E + 4096 + E / 64);
  c.edgeUp.reserve(E + 4096 + E / 64);
  c.col.resize(E);
  c.metric.resize(E);
  c.linkId.resize(E);
  c.twin.resize(E);
  c.linkRank.resize(E);
  c.edgeUp.resize(E);
  std::vector<uint32_t> side(c.links.size() * 2, kInf);
  parallelFor(V, [&](uint32_t lo, uint32_t hi) {
    for (uint32_t u = lo; u < hi; ++u) {
      auto& row = rows[u];
      std::sort(row.begin(), row.end(), [](const Ent& a, const Ent& b) {
        return a.v != b.v ? a.v < b.v : a.rank < b.rank;
      });
      size_t e = c.rowPtr[u];
      for (const auto& x : row) {
        const uint32_t lid = (*x.link)->snapLid;
        c.col[e] = x.v;
        c.metric[e] = x.metric;
        c.linkId[e] = lid;
        c.linkRank[e] = x.rank;
        c.edgeUp[e] = x.up;
        side[lid * 2ull + (x.low ? 0 : 1)] = (uint32_t)e;  // each (link, end) once
        ++e;
      }
    }
  });
  lap("rows sorted");
  parallelFor(V, [&](uint32_t lo, uint32_t hi) {
    for (size_t e = c.rowPtr[lo]; e < c.rowPtr[hi]; ++e) {
      const uint32_t lid = c.linkId[e];
      const uint32_t mine = side[lid * 2ull] == e ? 0u : 1u;
      c.twin[e] = side[lid * 2ull + (1u - mine)];
    }
  });
  lap("rows");
  c.rowMax = std::move(rowMax);
  csr_ = std::make_shared<Csr>(std::move(c));
  lap("move");
  snapVersion_ = version_;
  return *csr_;
}

uint32_t LinkState::linkIdOf(const Link& l) const {
  const uint32_t lid = l.snapLid;
  if (lid >= csr_->links.size() || csr_->links[lid].get() != &l)
    throw std::out_of_range("link not in the CSR snapshot");
  return lid;
}

// ---- device errors: degrade to the host path
template <class F>
decltype(auto) LinkState::guarded(F&& f) {
  if (guardDepth_) return f();  // an inner entry point: the outermost one handles it
  struct Depth {
    int& d;
    explicit Depth(int& x) : d(x) { ++d; }
    ~Depth() { --d; }
  };
  const uint64_t runs0 = spfRuns_;
  const size_t memo0 = memoMetric_.size() + memoHops_.size();
  // decision.spf_ms (LinkState.cpp:844,906-909): the call's time, charged to
  // the logical runs it made
  struct Timer {
    LinkState& ls;
    uint64_t runs0;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~Timer() {
      if (ls.spfRuns_ <= runs0) return;
      ls.counters_.spf_ms_samples += ls.spfRuns_ - runs0;
      ls.counters_.spf_ms_sum +=
          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  } timer{*this, runs0};
  try {
    Depth dp(guardDepth_);
    return f();
  } catch (const EngineError& e) {
    if (!degradeOnError_ || !engineOpened_) throw;
    onEngineError(e);
  }
  // runs memoised before the failure were made (and stay); the retry counts
  // its own
  spfRuns_ = runs0 + (memoMetric_.size() + memoHops_.size() - memo0);
  Depth dp(guardDepth_);
  return f();
}

void LinkState::onEngineError(const std::exception& e) {
  ++engineErrors_;
  lastEngineError_ = e.what();
  fprintf(stderr, "odl::LinkState(%s): engine error, continuing on the host path: %s\n",
          area_.c_str(), e.what());
  // the tracked selection's baseline leaves the device with the engine (a
  // device that cannot give it back: the next selectDelta reports `full`)
  trackPull();
  trackDropDev();
  for (AreasTracker* t : areasTrackers_) t->pull();  // their baseline leaves with the engine too
  dropSweep();
  if (multi_) ospf_multi_close(multi_);
  else if (engine_) ospf_close(engine_);
  multi_ = nullptr;
  engine_ = nullptr;
  engineVersion_ = 0;
  hostOnly_ = true;
  degraded_ = true;
}

void LinkState::injectEngineError(uint32_t after) {
  injectAfter_ = after;
  if (engine_) {
    ospf_inject_error(engine_, after);
    injectAfter_ = 0;
  }
}

const SpfResult& LinkState::getSpfResult(const std::string& node, bool useLinkMetric) {
  return guarded([&]() -> const SpfResult& { return getSpfResultImpl(node, useLinkMetric); });
}
void LinkState::prefetchSpf(const std::vector<std::string>& roots, bool useLinkMetric) {
  guarded([&] { prefetchSpfImpl(roots, useLinkMetric); });
}
std::vector<ospf_digest> LinkState::spfDigests(const std::vector<std::string>& roots,
                                               bool useLinkMetric) {
  return guarded([&] { return spfDigestsImpl(roots, useLinkMetric); });
}
void LinkState::prefetchAllSources(bool useLinkMetric) {
  guarded([&] { prefetchAllSourcesImpl(useLinkMetric); });
}
std::vector<ospf_digest> LinkState::allSourcesDigests(bool useLinkMetric) {
  return guarded([&] { return allSourcesDigestsImpl(useLinkMetric); });
}
const std::vector<Path>& LinkState::getKthPaths(const std::string& src, const std::string& dst,
                                                size_t k) {
  return guarded([&]() -> const std::vector<Path>& { return getKthPathsImpl(src, dst, k); });
}
void LinkState::prefetchKsp2(const std::string& src, const std::vector<std::string>& dsts) {
  guarded([&] { prefetchKsp2Impl(src, dsts); });
}

void LinkState::startOpen(size_t nodes) {
  if (hostOnly_ || engine_ || opener_.joinable() || devices_.size() != 1 ||
      knob_flag(Knob::ODL_NO_PREOPEN))
    return;
  // the warm-up: one link, one root (a warm-up graph as large as the
  // ingested one -- a hypercube, to size the batch path's buffers too -- cost
  // more on the first getSpfResult's path than the ~14 ms it saved there)
  (void)nodes;
  constexpr uint32_t V = 2;
  try {
    opener_ = std::thread([this, dev = device_] {
      ospf_ctx* c = nullptr;
      if (ospf_open(dev, &c) != OSPF_OK) return;
      const std::vector<uint32_t> rp{0, 1, 2}, col{1, 0}, one{1, 1}, lid{0, 0}, twin{1, 0};
      const std::vector<uint8_t> up{1, 1};
      const uint32_t E = 2;
      ospf_csr g{};
      g.n_nodes = V;
      g.n_edges = E;
      g.row_ptr = rp.data();
      g.col = col.data();
      g.metric = one.data();
      g.link_id = lid.data();
      g.twin = twin.data();
      g.edge_up = up.data();
      uint32_t root = 0;
      std::vector<uint32_t> dist(V), nh(V);
      if (ospf_load_graph(c, &g, 0) != OSPF_OK ||
          ospf_sssp_batch(c, &root, 1, nullptr, OSPF_WANT_DIST | OSPF_WANT_NH, 1, dist.data(),
                          nh.data(), nullptr) != OSPF_OK) {
        ospf_close(c);
        return;
      }
      openerCtx_ = c;
    });
  } catch (const std::system_error&) {  // no thread: the engine opens on first use
  }
}

void LinkState::joinOpen() {
  if (!opener_.joinable()) return;
  opener_.join();
  if (!openerCtx_) return;  // failed: ensureEngine opens (and reports) as before
  if (engine_ || hostOnly_) {
    ospf_close(openerCtx_);
  } else {
    engine_ = openerCtx_;
    engineOpened_ = true;
    engineVersion_ = 0;  // the warm-up graph: the snapshot loads on first use
  }
  openerCtx_ = nullptr;
}

void LinkState::ensureEngine() {
  snapshot();
  joinOpen();
  const auto t0 = std::chrono::steady_clock::now();
  const bool opening = !engine_, loading = engineVersion_ != snapVersion_;
  if (!engine_) {
    int rc = OSPF_OK;
    if (devices_.size() > 1) {
      rc = ospf_multi_open(devices_.data(), (uint32_t)devices_.size(), &multi_);
      if (rc == OSPF_OK) engine_ = ospf_multi_ctx(multi_, 0);
    } else {
      rc = ospf_open(device_, &engine_);
    }
    if (rc != OSPF_OK) {
      engine_ = nullptr;
      multi_ = nullptr;
      throw EngineError(rc, "ospf_open failed (no MI355X device / HIP runtime?)");
    }
    engineOpened_ = true;
  }
  if (injectAfter_) {
    ospf_inject_error(engine_, injectAfter_);
    injectAfter_ = 0;
  }
  const auto tOpen = std::chrono::steady_clock::now();
  if (engineVersion_ != snapVersion_) {
    dropSweep();
    ospf_csr g{};
    g.n_nodes = (uint32_t)csr_->names.size();
    g.n_edges = (uint32_t)csr_->col.size();
    g.row_ptr = csr_->rowPtr.data();
    g.col = csr_->col.data();
    g.metric = csr_->metric.data();
    g.link_id = csr_->linkId.data();
    g.twin = csr_->twin.data();
    g.edge_up = csr_->edgeUp.data();
    g.no_transit = csr_->noTransit.data();
    g.link_rank = csr_->linkRank.data();
    int rc = multi_ ? ospf_multi_load_graph(multi_, &g, snapVersion_)
                    : ospf_load_graph(engine_, &g, snapVersion_);
    if (rc != OSPF_OK)
      throw EngineError(rc, multi_ ? ospf_multi_last_error(multi_) : ospf_last_error(engine_));
    ++topoStats_.loads;
    engineVersion_ = snapVersion_;
  }
  if ((opening || loading) && knob_flag(Knob::ODL_SPF_TIMING))
    fprintf(stderr, "ensure_engine open=%d load=%d open_ms=%.3f load_ms=%.3f\n", opening, loading,
            std::chrono::duration<double, std::milli>(tOpen - t0).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tOpen).count());
}

void LinkState::dropSweep() {
  if (sweep_) ospf_sweep_destroy(sweep_);
  if (msweep_) ospf_msweep_destroy(msweep_);
  sweep_ = nullptr;
  msweep_ = nullptr;
  sweepVersion_ = 0;
}

bool LinkState::sweepHas(bool useLinkMetric) const {
  return (sweep_ || msweep_) && sweepVersion_ == snapVersion_ && sweepMetric_ == useLinkMetric &&
         snapVersion_ == version_;
}

void LinkState::prefetchAllSourcesImpl(bool useLinkMetric) {
  snapshot();
  if (sweepHas(useLinkMetric)) return;
  if (hostRun(useLinkMetric)) {  // outside the engine contract: the reference algorithm
    prefetchSpf(csr_->names, useLinkMetric);
    return;
  }
  ensureEngine();
  dropSweep();
  ospf_sweep_opts o{};
  // one run per snapshot: nothing to replay, and the create makes no run of
  // its own (OSPF_SWEEP_DEFER): the run below is the only one
  o.flags = (useLinkMetric ? 0u : OSPF_HOP_COUNT) | OSPF_SWEEP_DEFER;
  o.mode = OSPF_SWEEP_AUTO;
  o.hip_graph = 0;
  int rc;
  ospf_sweep_info info{};
  if (multi_) {
    rc = ospf_msweep_create(multi_, &o, &msweep_);
    if (rc == OSPF_OK) rc = ospf_msweep_run(msweep_);
    if (rc != OSPF_OK) {
      const std::string m = ospf_multi_last_error(multi_);
      dropSweep();
      throw EngineError(rc, m);
    }
    ospf_sweep_get_info(ospf_msweep_part(msweep_, 0), &info);
    sweepStats_.devices = ospf_multi_size(multi_);
  } else {
    // the serial prefix of the run starts while the plan is still built
    o.flags |= OSPF_SWEEP_EARLY_START;
    rc = ospf_sweep_create(engine_, &o, &sweep_);
    bool runErr = false;  // ospf_sweep_run reports through the sweep's own error
    if (rc == OSPF_OK) runErr = (rc = ospf_sweep_run(sweep_, nullptr)) != OSPF_OK;
    if (rc == OSPF_OK) rc = ospf_sync(engine_, nullptr);
    if (rc != OSPF_OK) {
      const std::string m = runErr ? ospf_sweep_last_error(sweep_) : ospf_last_error(engine_);
      dropSweep();
      throw EngineError(rc, m);
    }
    ospf_sweep_get_info(sweep_, &info);
    sweepStats_.devices = 1;
  }
  sweepVersion_ = snapVersion_;
  sweepMetric_ = useLinkMetric;
  spfRuns_ += csr_->names.size();  // every node's runSpf, once
  ++sweepStats_.sweeps;
  sweepStats_.mode = info.mode;
  sweepStats_.hip_graph = info.hip_graph;
}

void LinkState::sweepRows(const std::vector<uint32_t>& roots, uint32_t W,
                          std::vector<uint32_t>& dist, std::vector<uint32_t>& nh) {
  const size_t V = csr_->names.size();
  dist.assign(roots.size() * V, kInf);
  nh.assign(roots.size() * V * W, 0);
  if (sweep_) {
    const int rc = ospf_sweep_copy_rows(sweep_, roots.data(), (uint32_t)roots.size(), W,
                                        dist.data(), nh.data());
    if (rc != OSPF_OK) throw EngineError(rc, ospf_sweep_last_error(sweep_));
  } else {
    for (size_t i = 0; i < roots.size(); ++i) {
      uint32_t slot = 0;
      int rc = ospf_msweep_owner(msweep_, roots[i], &slot);
      if (rc != OSPF_OK)
        throw EngineError(rc, "all-sources sweep: no part owns node " + csr_->names[roots[i]]);
      ospf_sweep* part = ospf_msweep_part(msweep_, slot);
      rc = ospf_sweep_copy_rows(part, &roots[i], 1, W, dist.data() + i * V, nh.data() + i * V * W);
      if (rc != OSPF_OK) throw EngineError(rc, ospf_sweep_last_error(part));
    }
  }
  sweepStats_.rows_copied += roots.size();
}

std::vector<ospf_digest> LinkState::allSourcesDigestsImpl(bool useLinkMetric) {
  snapshot();
  const size_t V = csr_->names.size();
  if (hostRun(useLinkMetric)) return spfDigests(csr_->names, useLinkMetric);
  prefetchAllSources(useLinkMetric);
  std::vector<ospf_digest> out(V);
  if (msweep_) {
    const int rc = ospf_msweep_digests(msweep_, out.data());
    if (rc != OSPF_OK) throw EngineError(rc, ospf_multi_last_error(multi_));
    return out;
  }
  const std::vector<uint32_t> roots = ownedRoots();
  std::vector<ospf_digest> tmp(roots.size());
  const int rc = ospf_sweep_digests_host(sweep_, tmp.data());
  if (rc != OSPF_OK) throw EngineError(rc, ospf_sweep_last_error(sweep_));
  for (size_t i = 0; i < roots.size(); ++i) out[roots[i]] = tmp[i];
  return out;
}

std::vector<uint32_t> LinkState::ownedRoots() const {
  ospf_sweep_info info{};
  ospf_sweep_get_info(sweep_, &info);
  std::vector<uint32_t> roots(info.n_roots);
  ospf_sweep_roots(sweep_, roots.data());
  return roots;
}

// ---------------------------------------------------------------- select: the shared host steps
namespace {

using Lists = std::vector<std::vector<uint32_t>>;  // one list per prefix

// the distinct neighbours of a root, ascending: the next-hop bit order (nhWordsFor)
std::vector<uint32_t> distinctNbrs(const LinkState::Csr& cs, uint32_t root) {
  std::vector<uint32_t> out;
  for (uint32_t e = cs.rowPtr[root]; e < cs.rowPtr[root + 1]; ++e) {
    const uint32_t v = cs.col[e];
    if (v != root && (out.empty() || out.back() != v)) out.push_back(v);
  }
  return out;
}

// the slot (bit) of neighbour `id` in nbrs, nbrs.size() when it is none
uint32_t slotOf(const std::vector<uint32_t>& nbrs, uint32_t id) {
  const auto it = std::lower_bound(nbrs.begin(), nbrs.end(), id);
  return (uint32_t)((it != nbrs.end() && *it == id ? it : nbrs.end()) - nbrs.begin());
}

// A root's links as route selection sees them: its distinct neighbours and,
// per slot, the links r - k getNextHopsThrift emits: up, at the smallest
// metric r advertises towards k (every up link under hop count)
struct LinkView {
  std::vector<uint32_t> nbrs, c;
};
LinkView linkView(const LinkState::Csr& cs, uint32_t r, bool useLinkMetric) {
  LinkView v;
  v.nbrs = distinctNbrs(cs, r);
  v.c.assign(v.nbrs.size(), 0);
  std::vector<uint32_t> minw(v.nbrs.size(), kInf);
  for (int pass = 0; pass < 2; ++pass)
    for (uint32_t e = cs.rowPtr[r]; e < cs.rowPtr[r + 1]; ++e) {
      if (cs.col[e] == r || !cs.edgeUp[e]) continue;
      const uint32_t k = slotOf(v.nbrs, cs.col[e]);
      if (!pass) minw[k] = std::min(minw[k], cs.metric[e]);
      else if (!useLinkMetric || cs.metric[e] == minw[k]) ++v.c[k];
    }
  return v;
}

// next-hop names -> bits of `words` (W of them) by slot in nbrs; onNew(k) for
// every bit k this call set
template <class OnNew>
void setNextHopBits(uint32_t* words, uint32_t W, const std::vector<uint32_t>& nbrs,
                    const std::unordered_map<std::string, uint32_t>& ids,
                    const std::unordered_set<std::string>& nextHopNames, OnNew&& onNew) {
  for (const auto& nhName : nextHopNames) {
    const uint32_t k = slotOf(nbrs, ids.at(nhName));
    if (k == nbrs.size() || k / 32 >= W || (words[k / 32] >> (k % 32) & 1u)) continue;
    words[k / 32] |= 1u << (k % 32);
    onNew(k);
  }
}
void setNextHopBits(uint32_t* words, uint32_t W, const std::vector<uint32_t>& nbrs,
                    const std::unordered_map<std::string, uint32_t>& ids,
                    const std::unordered_set<std::string>& nextHopNames) {
  setNextHopBits(words, W, nbrs, ids, nextHopNames, [](uint32_t) {});
}

// the links behind the set bits of `words`: an IP route's next-hop links
uint32_t linksOf(const uint32_t* words, uint32_t W, const std::vector<uint32_t>& c) {
  uint32_t n = 0;
  for (uint32_t k = 0; k < c.size() && k / 32 < W; ++k)
    if (words[k / 32] >> (k % 32) & 1u) n += c[k];
  return n;
}

// createRouteForPrefix's first steps for one root and one prefix of a single
// area (SpfSolver.cpp:229-244, 649-676, 709-731): the announcers the root
// reaches, of them the best class S, and S without its drained members
// unless all are drained (Sf); positions into ann, ascending; d: the distance
// of each reached announcer. False: none reached.
struct BestClass {
  std::vector<Metric> d;
  std::vector<size_t> S, Sf;
};
bool bestClass(const SpfResult& res, const LinkState::Csr& cs, const std::vector<uint32_t>& ann,
               const std::vector<uint32_t>& pref, BestClass& b) {
  std::vector<size_t> R;
  b.d.assign(ann.size(), 0);
  b.S.clear();
  b.Sf.clear();
  uint32_t top = kInf;
  for (size_t i = 0; i < ann.size(); ++i) {
    const auto it = res.find(cs.names[ann[i]]);
    if (it == res.end()) continue;
    b.d[i] = it->second.metric();
    R.push_back(i);
    top = std::min(top, pref[i]);
  }
  for (size_t i : R)
    if (pref[i] == top) b.S.push_back(i);
  for (size_t i : b.S)
    if (!cs.noTransit[ann[i]]) b.Sf.push_back(i);
  if (b.Sf.empty()) b.Sf = b.S;
  return !R.empty();
}

// bestNodeArea's node: the smallest id of S (ann ascends), or the root itself
uint32_t bestOf(const std::vector<size_t>& S, const std::vector<uint32_t>& ann, uint32_t r) {
  for (size_t i : S)
    if (ann[i] == r) return r;
  return ann[S.front()];
}

// per-prefix lists -> one flat list (and, with `off`, where each prefix starts)
std::vector<uint32_t> flatten(const Lists& lists, std::vector<uint32_t>* off = nullptr) {
  std::vector<uint32_t> flat;
  if (off) off->assign(1, 0);
  for (const auto& l : lists) {
    flat.insert(flat.end(), l.begin(), l.end());
    if (off) off->push_back((uint32_t)flat.size());
  }
  return flat;
}

// rows in the sweep's owned-roots order -> rows by node id, `per` words each
void scatterOwned(const std::vector<uint32_t>& roots, const std::vector<uint32_t>& src,
                  std::vector<uint32_t>& dst, size_t per) {
  for (size_t i = 0; i < roots.size(); ++i)
    std::copy(src.begin() + i * per, src.begin() + (i + 1) * per, dst.begin() + roots[i] * per);
}

// rows `ids` of src ([.][cells][from]) -> dst ([ids.size()][cells][to], to >=
// from: the tail of each cell stays as it is)
void gatherRows(const std::vector<uint32_t>& ids, size_t cells, const std::vector<uint32_t>& src,
                size_t from, std::vector<uint32_t>& dst, size_t to) {
  for (size_t i = 0; i < ids.size(); ++i)
    for (size_t p = 0; p < cells; ++p)
      std::copy(src.begin() + (ids[i] * cells + p) * from,
                src.begin() + (ids[i] * cells + p + 1) * from, dst.begin() + (i * cells + p) * to);
}

// a route is programmed when it has next-hop links and at least minNexthop
// of them (SpfSolver.cpp:990-1000)
bool isInstalled(uint32_t links, uint32_t need) { return links > 0 && need <= links; }
void markInstalled(const std::vector<uint32_t>& links, const std::vector<uint32_t>& need,
                   std::vector<uint8_t>& installed) {
  installed.resize(links.size());
  for (size_t i = 0; i < links.size(); ++i) installed[i] = isInstalled(links[i], need[i]);
}

// the next-hop width of a call: nhWords, or `need` when it is 0; one below `need` throws
constexpr const char* kWidest = " below the widest node's ";
constexpr const char* kBaseline = " below the baseline's ";
uint32_t wordsFor(const char* who, uint32_t nhWords, uint32_t need, const char* what) {
  const uint32_t W = nhWords ? nhWords : need;
  if (W < need)
    throw std::invalid_argument(std::string(who) + ": nhWords " + std::to_string(W) + what +
                                std::to_string(need));
  return W;
}

// results of `rows` nodes, P prefixes and W words: nothing reached anywhere
LinkState::SelectResult selectResult(size_t rows, size_t P, uint32_t W) {
  LinkState::SelectResult r;
  r.prefixes = (uint32_t)P;
  r.words = W;
  r.metric.assign(rows * P, kInf);
  r.count.assign(rows * P, 0);
  r.nh.assign(rows * P * W, 0);
  return r;
}
LinkState::PolicyResult policyResult(size_t rows, size_t P, uint32_t W) {
  LinkState::PolicyResult r;
  r.prefixes = (uint32_t)P;
  r.words = W;
  r.metric.assign(rows * P, kInf);
  r.best.assign(rows * P, kInf);
  for (auto* v : {&r.count, &r.links, &r.need}) v->assign(rows * P, 0);
  r.nh.assign(rows * P * W, 0);
  r.installed.assign(rows * P, 0);
  return r;
}
ospf_select_pout pout(LinkState::PolicyResult& r) {
  return {r.metric.data(), r.count.data(), r.nh.data(), r.links.data(), r.need.data(), r.best.data()};
}

}  // namespace

uint32_t LinkState::selectWords() {
  snapshot();
  uint32_t W = 1;
  for (uint32_t v = 0; v < csr_->names.size(); ++v) W = std::max(W, nhWordsFor(v));
  return W;
}

Lists LinkState::annIds(const std::vector<std::vector<std::string>>& prefixes) const {
  // names -> ids: unknown names dropped, ascending and distinct per prefix
  Lists ann(prefixes.size());
  for (size_t p = 0; p < prefixes.size(); ++p) {
    for (const auto& nm : prefixes[p]) {
      const auto it = csr_->ids.find(nm);
      if (it != csr_->ids.end()) ann[p].push_back(it->second);
    }
    std::sort(ann[p].begin(), ann[p].end());
    ann[p].erase(std::unique(ann[p].begin(), ann[p].end()), ann[p].end());
  }
  return ann;
}

LinkState::SelectResult LinkState::allSourcesSelect(
    const std::vector<std::vector<std::string>>& prefixes, bool useLinkMetric, uint32_t nhWords) {
  snapshot();
  const uint32_t W = wordsFor("allSourcesSelect", nhWords, selectWords(), kWidest);
  const Lists ann = annIds(prefixes);
  return guarded([&] { return allSourcesSelectImpl(ann, useLinkMetric, W); });
}

LinkState::SelectResult LinkState::allSourcesSelectImpl(const Lists& ann, bool useLinkMetric,
                                                        uint32_t W) {
  snapshot();
  const size_t V = csr_->names.size(), P = ann.size();
  SelectResult out = selectResult(V, P, W);
  if (!V || !P) return out;
  if (hostRun(useLinkMetric)) {
    // the reference loop (SpfSolver.cpp:1058-1086) over getSpfResult of every node
    for (uint32_t r = 0; r < V; ++r) {
      const SpfResult& res = getSpfResult(csr_->names[r], useLinkMetric);
      const std::vector<uint32_t> nbrs = nbrsOf(r);
      for (size_t p = 0; p < P; ++p) {
        Metric shortest = std::numeric_limits<Metric>::max();
        std::vector<uint32_t> minCost;
        for (uint32_t a : ann[p]) {
          const auto it = res.find(csr_->names[a]);
          if (it == res.end()) continue;
          const Metric d = it->second.metric();
          if (shortest >= d) {
            if (shortest > d) {
              shortest = d;
              minCost.clear();
            }
            minCost.push_back(a);
          }
        }
        if (minCost.empty()) continue;
        out.metric[r * P + p] = (uint32_t)shortest;
        out.count[r * P + p] = (uint32_t)minCost.size();
        for (uint32_t a : minCost)
          setNextHopBits(out.nh.data() + (r * P + p) * W, W, nbrs, csr_->ids,
                         res.at(csr_->names[a]).nextHops());
      }
    }
    return out;
  }
  prefetchAllSources(useLinkMetric);
  std::vector<uint32_t> off;
  const std::vector<uint32_t> nodes = flatten(ann, &off);
  const ospf_select_table t{(uint32_t)P, off.data(), nodes.data()};
  if (msweep_) {
    const int rc = ospf_msweep_select(msweep_, &t, W, out.metric.data(), out.count.data(),
                                      out.nh.data());
    if (rc != OSPF_OK) throw EngineError(rc, ospf_multi_last_error(multi_));
    return out;
  }
  const std::vector<uint32_t> roots = ownedRoots();
  std::vector<uint32_t> m(roots.size() * P), k(roots.size() * P), nh(roots.size() * P * W);
  const int rc = ospf_sweep_select(sweep_, &t, W, m.data(), k.data(), nh.data());
  if (rc != OSPF_OK) throw EngineError(rc, ospf_sweep_last_error(sweep_));
  scatterOwned(roots, m, out.metric, P);
  scatterOwned(roots, k, out.count, P);
  scatterOwned(roots, nh, out.nh, P * W);
  return out;
}

// ---------------------------------------------------------------- select policy
void LinkState::policyTable(const std::vector<std::vector<std::string>>& prefixes,
                            const std::vector<std::vector<SelectAttr>>& attrs, const char* who,
                            std::vector<std::vector<uint32_t>>& ann,
                            std::vector<std::vector<uint32_t>>& pref,
                            std::vector<std::vector<uint32_t>>& mnh,
                            std::vector<std::vector<uint32_t>>* pos) const {
  if (attrs.size() != prefixes.size())
    throw std::invalid_argument(std::string(who) + ": one attribute list per prefix");
  const size_t P = prefixes.size();
  ann.assign(P, {});
  pref.assign(P, {});
  mnh.assign(P, {});
  if (pos) pos->assign(P, {});
  for (size_t p = 0; p < P; ++p) {
    if (attrs[p].size() != prefixes[p].size())
      throw std::invalid_argument(std::string(who) + ": one attribute set per announcer");
    // names -> ids: unknown names dropped with their attributes, the first
    // occurrence of a name counts; ascending by id
    std::vector<std::pair<uint32_t, size_t>> ent;  // (id, position in the prefix's list)
    for (size_t i = 0; i < prefixes[p].size(); ++i) {
      const auto it = csr_->ids.find(prefixes[p][i]);
      if (it != csr_->ids.end()) ent.emplace_back(it->second, i);
    }
    std::sort(ent.begin(), ent.end());
    ent.erase(std::unique(ent.begin(), ent.end(),
                          [](const auto& a, const auto& b) { return a.first == b.first; }),
              ent.end());
    std::vector<SelectAttr> kept;
    for (const auto& e : ent) kept.push_back(attrs[p][e.second]);
    pref[p] = classRanks(kept);
    for (size_t i = 0; i < ent.size(); ++i) {
      ann[p].push_back(ent[i].first);
      mnh[p].push_back(clampedMinNexthop(kept[i]));
      if (pos) (*pos)[p].push_back((uint32_t)ent[i].second);
    }
  }
}

// the dense class rank of each entry among the given ones: (pathPreference,
// sourcePreference) descending, distance ascending
// (selectRoutes(SHORTEST_DISTANCE), LsdbUtil.cpp:841-883)
std::vector<uint32_t> LinkState::classRanks(const std::vector<SelectAttr>& attrs) {
  using Cls = std::array<int64_t, 3>;
  auto cls = [](const SelectAttr& a) { return Cls{a.pathPreference, a.sourcePreference, a.distance}; };
  auto better = [](const Cls& a, const Cls& b) {
    if (a[0] != b[0]) return a[0] > b[0];
    if (a[1] != b[1]) return a[1] > b[1];
    return a[2] < b[2];
  };
  std::vector<Cls> classes;
  for (const auto& a : attrs) classes.push_back(cls(a));
  std::sort(classes.begin(), classes.end(), better);
  classes.erase(std::unique(classes.begin(), classes.end()), classes.end());
  std::vector<uint32_t> out;
  for (const auto& a : attrs)
    out.push_back((uint32_t)(std::lower_bound(classes.begin(), classes.end(), cls(a), better) -
                             classes.begin()));
  return out;
}

uint32_t LinkState::clampedMinNexthop(const SelectAttr& a) {
  return a.minNexthop ? (uint32_t)std::clamp<int64_t>(*a.minNexthop, 0, 0xFFFFFFFFll) : 0u;
}

// ---------------------------------------------------------------- select across areas
// the areas by name and the engine's table, as allAreasSelect maps them
struct LinkState::AreasMap {
  std::vector<LinkState*> ar;
  std::vector<std::vector<uint32_t>> gid;
  std::vector<uint32_t> off, tnode, tarea, tpref, tmnh;
};

LinkState::AreasResult LinkState::allAreasSelectImpl(
    const std::vector<LinkState*>& given, const std::vector<std::vector<AreaEntry>>& prefixes,
    bool useLinkMetric, AreasWhat what, AreasMap* map) {
  if (given.empty() || given.size() > 32)
    throw std::invalid_argument("allAreasSelect: 1 .. 32 areas");
  // the areas by name
  AreasResult out;
  out.order.resize(given.size());
  for (size_t i = 0; i < given.size(); ++i) {
    if (!given[i]) throw std::invalid_argument("allAreasSelect: null area");
    out.order[i] = (uint32_t)i;
  }
  std::sort(out.order.begin(), out.order.end(),
            [&](uint32_t a, uint32_t b) { return given[a]->area_ < given[b]->area_; });
  std::vector<LinkState*> ar;
  for (uint32_t i : out.order) ar.push_back(given[i]);
  const size_t A = ar.size(), P = prefixes.size();
  for (size_t a = 1; a < A; ++a)
    if (ar[a]->area_ == ar[a - 1]->area_)
      throw std::invalid_argument("allAreasSelect: area " + ar[a]->area_ + " given twice");
  // the name union and each area's global ids
  for (LinkState* ls : ar) {
    ls->snapshot();
    out.names.insert(out.names.end(), ls->csr_->names.begin(), ls->csr_->names.end());
  }
  std::sort(out.names.begin(), out.names.end());
  out.names.erase(std::unique(out.names.begin(), out.names.end()), out.names.end());
  const size_t G = out.names.size();
  std::vector<std::vector<uint32_t>> gid(A);
  for (size_t a = 0; a < A; ++a)
    for (const auto& nm : ar[a]->csr_->names)
      gid[a].push_back((uint32_t)(std::lower_bound(out.names.begin(), out.names.end(), nm) -
                                  out.names.begin()));
  // the table: an entry of an unknown area throws (the reference reads
  // areaLinkStates.at(area)); a node unknown to its area is dropped with its
  // attributes, of a (node, area) given twice the first counts; ascending in
  // (node, area); class ranks and clamped thresholds over the kept entries
  struct Ent {
    uint32_t node, area, loc;
    size_t at;
  };
  std::vector<uint32_t> off(P + 1, 0), tnode, tarea, tloc, tpref, tmnh;
  for (size_t p = 0; p < P; ++p) {
    std::vector<Ent> ent;
    for (size_t i = 0; i < prefixes[p].size(); ++i) {
      const AreaEntry& e = prefixes[p][i];
      size_t a = 0;
      while (a < A && ar[a]->area_ != e.area) ++a;
      if (a == A) throw std::invalid_argument("prefix entry of unknown area " + e.area);
      const auto it = ar[a]->csr_->ids.find(e.node);
      if (it == ar[a]->csr_->ids.end()) continue;
      ent.push_back(Ent{gid[a][it->second], (uint32_t)a, it->second, i});
    }
    std::stable_sort(ent.begin(), ent.end(), [](const Ent& x, const Ent& y) {
      return x.node != y.node ? x.node < y.node : x.area < y.area;
    });
    ent.erase(std::unique(ent.begin(), ent.end(),
                          [](const Ent& x, const Ent& y) { return x.node == y.node && x.area == y.area; }),
              ent.end());
    std::vector<SelectAttr> kept;
    for (const auto& e : ent) kept.push_back(prefixes[p][e.at].attr);
    const std::vector<uint32_t> ranks = classRanks(kept);
    for (size_t i = 0; i < ent.size(); ++i) {
      tnode.push_back(ent[i].node);
      tarea.push_back(ent[i].area);
      tloc.push_back(ent[i].loc);
      tpref.push_back(ranks[i]);
      tmnh.push_back(clampedMinNexthop(kept[i]));
    }
    off[p + 1] = (uint32_t)tnode.size();
  }
  out.prefixes = (uint32_t)P;
  out.words.resize(A);
  for (size_t a = 0; a < A; ++a) out.words[a] = ar[a]->selectWords();
  if (map) {
    map->ar = ar;
    map->gid = gid;
    map->off = off;
    map->tnode = tnode;
    map->tarea = tarea;
    map->tpref = tpref;
    map->tmnh = tmnh;
  }
  if (what == AreasWhat::kMapOnly) return out;
  out.nh.resize(A);
  for (size_t a = 0; a < A; ++a)
    out.nh[a].assign(ar[a]->csr_->names.size() * P * out.words[a], 0);
  out.metric.assign(G * P, kInf);
  out.best.assign(G * P, kInf);
  for (auto* v : {&out.count, &out.links, &out.need, &out.areas}) v->assign(G * P, 0);
  out.installed.assign(G * P, 0);
  if (!G || !P) return out;
  // the device path: every area on the engine, on one device of its own
  auto deviceOk = [&] {
    for (LinkState* ls : ar)
      if (ls->hostRun(useLinkMetric) || ls->devices_.size() > 1 || ls->device_ != ar[0]->device_)
        return false;
    return true;
  };
  if (what == AreasWhat::kAny && deviceOk()) {
    // re-sweep the areas whose version moved (a device error there degrades
    // that area: the host path below then answers)
    for (LinkState* ls : ar) ls->prefetchAllSources(useLinkMetric);
  }
  if (what == AreasWhat::kAny && deviceOk()) {
    bool swept = true;
    for (LinkState* ls : ar) swept = swept && ls->sweep_ && ls->sweepHas(useLinkMetric);
    if (swept) {
      std::vector<ospf_sweep*> sw;
      std::vector<const uint32_t*> gp;
      std::vector<uint32_t*> nhp;
      for (size_t a = 0; a < A; ++a) {
        sw.push_back(ar[a]->sweep_);
        gp.push_back(gid[a].data());
        nhp.push_back(out.nh[a].data());
      }
      const ospf_areas_table t{(uint32_t)A,     sw.data(),    gp.data(),    (uint32_t)G,
                               (uint32_t)P,     off.data(),   tnode.data(), tarea.data(),
                               tpref.data(),    tmnh.data()};
      const ospf_areas_pout o{out.metric.data(), out.count.data(), out.links.data(),
                              out.need.data(),   out.best.data(),  out.areas.data(),
                              nhp.data(),        out.words.data()};
      const int rc = ospf_areas_select_policy(&t, &o);
      if (rc == OSPF_OK) {
        out.onDevice = true;
        markInstalled(out.links, out.need, out.installed);
        return out;
      }
      const EngineError err(rc, ospf_sweep_last_error(sw[0]));
      // a device error (or the device out of memory) sends every area to its
      // host path, as an error inside one LinkState's own call does: they
      // share the device. All of them or none: an area that may not degrade
      // makes the call throw with no area touched. Any other code (a contract
      // or LDS-size refusal) is no fault of the device: this call alone is
      // answered on the host.
      if (rc == OSPF_E_DEVICE || rc == OSPF_E_NOMEM) {
        for (LinkState* ls : ar)
          if (!ls->degradeOnError_ || !ls->engineOpened_) throw err;
        for (LinkState* ls : ar) ls->onEngineError(err);
      }
    }
  }
  // the host path: the same steps over every area's getSpfResult
  for (uint32_t g = 0; g < G; ++g) {
    const std::string& me = out.names[g];
    struct Mine {
      const SpfResult* res = nullptr;
      uint32_t la = kInf;
      LinkView links;
    };
    std::vector<Mine> mine(A);
    for (size_t a = 0; a < A; ++a) {
      LinkState& ls = *ar[a];
      const auto it = ls.csr_->ids.find(me);
      if (it == ls.csr_->ids.end()) continue;
      Mine& m = mine[a];
      m.la = it->second;
      m.res = &ls.getSpfResult(me, useLinkMetric);
      m.links = linkView(*ls.csr_, m.la, useLinkMetric);
    }
    for (size_t p = 0; p < P; ++p) {
      const uint32_t lo = off[p], hi = off[p + 1];
      auto nameOf = [&](uint32_t k) -> const std::string& { return out.names[tnode[k]]; };
      // 1. reached in the entry's own area; 2. the best class
      std::vector<uint32_t> R, S, Sf;
      uint32_t top = kInf;
      for (uint32_t k = lo; k < hi; ++k) {
        const Mine& m = mine[tarea[k]];
        if (!m.res || !m.res->count(nameOf(k))) continue;
        R.push_back(k);
        top = std::min(top, tpref[k]);
      }
      if (R.empty()) continue;
      for (uint32_t k : R)
        if (tpref[k] == top) S.push_back(k);
      // 3. the drain filter, by the entry's own area
      for (uint32_t k : S)
        if (!ar[tarea[k]]->csr_->noTransit[tloc[k]]) Sf.push_back(k);
      if (Sf.empty()) Sf = S;
      // 4. / 5. per area of g with an entry of its own: the nodes of all of Sf
      const size_t cell = (size_t)g * P + p;
      Metric shortest = std::numeric_limits<Metric>::max();
      std::vector<std::pair<size_t, std::vector<const std::string*>>> won;
      for (size_t a = 0; a < A; ++a) {
        const Mine& m = mine[a];
        if (!m.res) continue;
        bool own = false;
        for (uint32_t k : Sf) own = own || tarea[k] == a;
        if (!own) continue;
        Metric ma = std::numeric_limits<Metric>::max();
        std::vector<const std::string*> L;
        uint32_t prev = kInf;
        for (uint32_t k : Sf) {
          if (tnode[k] == prev) continue;  // each node once
          prev = tnode[k];
          const auto it = m.res->find(nameOf(k));
          if (it == m.res->end()) continue;
          const Metric d = it->second.metric();
          if (d < ma) {
            ma = d;
            L.clear();
          }
          if (d == ma) L.push_back(&nameOf(k));
        }
        if (L.empty() || ma > shortest) continue;
        if (ma < shortest) {
          shortest = ma;
          won.clear();
        }
        won.emplace_back(a, std::move(L));
      }
      // 6. outputs
      for (const auto& [a, L] : won) {
        const Mine& m = mine[a];
        const uint32_t W = out.words[a];
        uint32_t* words = out.nh[a].data() + ((size_t)m.la * P + p) * W;
        for (const std::string* d : L)
          setNextHopBits(words, W, m.links.nbrs, ar[a]->csr_->ids, m.res->at(*d).nextHops());
        out.links[cell] += linksOf(words, W, m.links.c);
        out.count[cell] += (uint32_t)L.size();
        out.areas[cell] |= 1u << a;
      }
      out.metric[cell] = (uint32_t)shortest;
      for (uint32_t k : Sf) out.need[cell] = std::max(out.need[cell], tmnh[k]);
      out.best[cell] = S.front() - lo;
      for (uint32_t k : S)
        if (tnode[k] == g) {
          out.best[cell] = k - lo;
          break;
        }
    }
  }
  markInstalled(out.links, out.need, out.installed);
  return out;
}

// ---------------------------------------------------------------- the areas tracker
LinkState::AreasResult LinkState::allAreasSelect(const std::vector<LinkState*>& given,
                                                 const std::vector<std::vector<AreaEntry>>& prefixes,
                                                 bool useLinkMetric) {
  return allAreasSelectImpl(given, prefixes, useLinkMetric, AreasWhat::kAny, nullptr);
}

std::unique_ptr<LinkState::AreasTracker> LinkState::trackAreasSelect(
    const std::vector<LinkState*>& areas, const std::vector<std::vector<AreaEntry>>& prefixes,
    bool useLinkMetric) {
  return std::make_unique<AreasTracker>(areas, prefixes, useLinkMetric);
}

LinkState::AreasTracker::AreasTracker(const std::vector<LinkState*>& areas,
                                      const std::vector<std::vector<AreaEntry>>& prefixes,
                                      bool useLinkMetric)
    : given_(areas), prefixes_(prefixes), ulm_(useLinkMetric) {
  baseline();  // throws on a bad argument: nothing registered yet
  for (LinkState* ls : given_) ls->areasTrackers_.push_back(this);
}

LinkState::AreasTracker::~AreasTracker() {
  for (LinkState* ls : given_) {
    auto& l = ls->areasTrackers_;
    l.erase(std::remove(l.begin(), l.end(), this), l.end());
  }
  if (st_) ospf_areastate_destroy(st_);
}

void LinkState::AreasTracker::remember(const AreasMap& m, const AreasResult& r) {
  names_ = r.names;
  order_ = r.order;
  words_ = r.words;
  gid_ = m.gid;
  const size_t A = m.ar.size();
  areaNames_.resize(A);
  nbrs_.resize(A);
  for (size_t a = 0; a < A; ++a) {
    areaNames_[a] = m.ar[a]->csr_->names;
    nbrs_[a].resize(areaNames_[a].size());
    for (uint32_t r0 = 0; r0 < nbrs_[a].size(); ++r0) nbrs_[a][r0] = m.ar[a]->nbrsOf(r0);
  }
}

bool LinkState::AreasTracker::namesMoved(const AreasMap& m) const {
  if (areaNames_.size() != m.ar.size()) return true;
  for (size_t a = 0; a < m.ar.size(); ++a)
    if (areaNames_[a] != m.ar[a]->csr_->names) return true;
  return false;
}

std::vector<ospf_sweep*> LinkState::AreasTracker::sweeps(const AreasMap& m) {
  auto deviceOk = [&] {
    for (LinkState* ls : m.ar)
      if (ls->hostRun(ulm_) || ls->devices_.size() > 1 || ls->device_ != m.ar[0]->device_)
        return false;
    return true;
  };
  std::vector<ospf_sweep*> sw;
  if (!deviceOk()) return sw;
  for (LinkState* ls : m.ar) ls->prefetchAllSources(ulm_);  // an error there degrades that area
  if (!deviceOk()) return sw;
  for (LinkState* ls : m.ar) {
    if (!ls->sweep_ || !ls->sweepHas(ulm_)) return {};
    sw.push_back(ls->sweep_);
  }
  return sw;
}

void LinkState::AreasTracker::engineFailed(const AreasMap& m, int rc, const std::string& msg) {
  // allAreasSelect's rule: a device error degrades every area or, when one may
  // not degrade, none and the error is thrown; another refusal sends only
  // this call to the host
  if (rc != OSPF_E_DEVICE && rc != OSPF_E_NOMEM) return;
  const EngineError err(rc, msg);
  for (LinkState* ls : m.ar)
    if (!ls->degradeOnError_ || !ls->engineOpened_) throw err;
  for (LinkState* ls : m.ar) ls->onEngineError(err);
}

void LinkState::AreasTracker::pull() {
  if (!st_) return;
  ospf_areastate* st = st_;
  st_ = nullptr;
  const size_t A = gid_.size(), G = names_.size(), P = prefixes_.size();
  AreasResult r;
  r.order = order_;
  r.names = names_;
  r.prefixes = (uint32_t)P;
  r.words = words_;
  for (auto* v : {&r.metric, &r.count, &r.links, &r.need, &r.best, &r.areas}) v->assign(G * P, 0);
  std::vector<std::vector<uint32_t>> byg(A);
  std::vector<uint32_t*> nhp;
  for (size_t a = 0; a < A; ++a) {
    byg[a].assign(G * P * words_[a], 0);
    nhp.push_back(byg[a].data());
  }
  std::vector<uint32_t> roots(G);
  for (uint32_t g = 0; g < G; ++g) roots[g] = g;
  const ospf_areas_pout o{r.metric.data(), r.count.data(), r.links.data(), r.need.data(),
                          r.best.data(),   r.areas.data(), nhp.data(),     words_.data()};
  const int rc = ospf_areastate_copy(st, roots.data(), (uint32_t)G, &o);
  ospf_areastate_destroy(st);
  hostOk_ = rc == OSPF_OK;
  if (!hostOk_) return;  // the baseline is lost: the next delta is `full`
  r.nh.resize(A);
  for (size_t a = 0; a < A; ++a) {
    const size_t row = P * words_[a];
    r.nh[a].assign(gid_[a].size() * row, 0);
    for (size_t i = 0; i < gid_[a].size(); ++i)
      std::copy(byg[a].begin() + gid_[a][i] * row, byg[a].begin() + (gid_[a][i] + 1) * row,
                r.nh[a].begin() + i * row);
  }
  markInstalled(r.links, r.need, r.installed);
  host_ = std::move(r);
}

void LinkState::AreasTracker::baseline() {
  if (st_) ospf_areastate_destroy(st_);
  st_ = nullptr;
  hostOk_ = false;
  AreasMap m;
  const AreasResult r = allAreasSelectImpl(given_, prefixes_, ulm_, AreasWhat::kMapOnly, &m);
  const std::vector<ospf_sweep*> sw = sweeps(m);
  if (!sw.empty()) {
    std::vector<const uint32_t*> gp;
    for (const auto& g : m.gid) gp.push_back(g.data());
    const ospf_areas_table t{(uint32_t)sw.size(),      sw.data(),       gp.data(),
                             (uint32_t)r.names.size(), r.prefixes,      m.off.data(),
                             m.tnode.data(),           m.tarea.data(),  m.tpref.data(),
                             m.tmnh.data()};
    ospf_areastate* st = nullptr;
    int rc = ospf_areastate_create(&t, &st);
    std::string msg = "ospf_areastate_create";
    if (rc == OSPF_OK && (rc = ospf_areastate_prime(st, sw.data())) != OSPF_OK) {
      msg = ospf_areastate_last_error(st);
      ospf_areastate_destroy(st);
    }
    if (rc == OSPF_OK) {
      st_ = st;
      remember(m, r);
      attrsMoved_ = false;
      return;
    }
    engineFailed(m, rc, msg);
  }
  host_ = allAreasSelectImpl(given_, prefixes_, ulm_, AreasWhat::kHostOnly, &m);
  hostOk_ = true;
  remember(m, host_);
  attrsMoved_ = false;
}

void LinkState::AreasTracker::setAttrs(const std::vector<std::vector<AreaEntry>>& prefixes) {
  if (prefixes.size() != prefixes_.size())
    throw std::invalid_argument("setAttrs: another number of prefixes than the tracked table");
  for (size_t p = 0; p < prefixes.size(); ++p) {
    if (prefixes[p].size() != prefixes_[p].size())
      throw std::invalid_argument("setAttrs: another number of entries than the tracked prefix");
    for (size_t i = 0; i < prefixes[p].size(); ++i)
      if (prefixes[p][i].node != prefixes_[p][i].node || prefixes[p][i].area != prefixes_[p][i].area)
        throw std::invalid_argument("setAttrs: the (node, area) entries differ from the tracked table");
  }
  prefixes_ = prefixes;
  attrsMoved_ = true;  // the device columns are replaced by the next delta()
}

void LinkState::AreasTracker::hostDiff(const AreasResult& now, const AreasMap& m, Delta& d) const {
  const AreasResult& old = host_;
  const size_t A = m.ar.size(), G = now.names.size(), P = now.prefixes;
  uint32_t sumW = 0;
  for (uint32_t w : now.words) sumW += w;
  std::vector<uint32_t> row(sumW);
  for (uint32_t g = 0; g < G; ++g) {
    // the root's id in each of its areas; rebased when a neighbour list moved
    std::vector<uint32_t> la(A, kInf);
    bool reb = false;
    for (size_t a = 0; a < A; ++a) {
      const auto it = std::lower_bound(m.gid[a].begin(), m.gid[a].end(), g);
      if (it == m.gid[a].end() || *it != g) continue;
      la[a] = (uint32_t)(it - m.gid[a].begin());
      reb = reb || nbrs_[a][la[a]] != m.ar[a]->nbrsOf(la[a]);
    }
    if (reb) {
      d.rebased.push_back(g);
      continue;
    }
    for (size_t p = 0; p < P; ++p) {
      const size_t c = (size_t)g * P + p;
      bool ch = old.metric[c] != now.metric[c] || old.count[c] != now.count[c] ||
                old.links[c] != now.links[c] || old.need[c] != now.need[c] ||
                old.best[c] != now.best[c] || old.areas[c] != now.areas[c];
      std::fill(row.begin(), row.end(), 0u);
      uint32_t base = 0;
      for (size_t a = 0; a < A; ++a) {
        const uint32_t Wn = now.words[a], Wo = old.words[a];
        if (la[a] != kInf) {
          const uint32_t* n = now.nh[a].data() + ((size_t)la[a] * P + p) * Wn;
          const uint32_t* o = old.nh[a].data() + ((size_t)la[a] * P + p) * Wo;
          for (uint32_t w = 0; w < std::max(Wn, Wo); ++w) {
            const uint32_t x = w < Wn ? n[w] : 0u, y = w < Wo ? o[w] : 0u;
            ch = ch || x != y;
            if (w < Wn) row[base + w] = x;
          }
        }
        base += Wn;
      }
      if (!ch) continue;
      d.changes.push_back(AreasChange{g, (uint32_t)p, now.metric[c], now.count[c], now.links[c],
                                      now.need[c], now.best[c], now.areas[c]});
      d.nh.insert(d.nh.end(), row.begin(), row.end());
    }
  }
}

LinkState::AreasTracker::Delta LinkState::AreasTracker::delta() {
  Delta d;
  AreasMap m;
  const AreasResult r = allAreasSelectImpl(given_, prefixes_, ulm_, AreasWhat::kMapOnly, &m);
  d.words = r.words;
  auto finish = [&] {
    d.installed.resize(d.changes.size());
    for (size_t i = 0; i < d.changes.size(); ++i)
      d.installed[i] = isInstalled(d.changes[i].links, d.changes[i].need);
  };
  if (namesMoved(m) || (!st_ && !hostOk_)) {
    baseline();
    d.words = words_;
    d.full = true;
    d.onDevice = st_ != nullptr;
    return d;
  }
  if (st_) {
    const std::vector<ospf_sweep*> sw = sweeps(m);  // may pull the baseline (an area's own error)
    if (st_ && !sw.empty()) {
      int rc = OSPF_OK;
      if (attrsMoved_) rc = ospf_areastate_set_policy(st_, m.tpref.data(), m.tmnh.data());
      if (rc == OSPF_OK) {
        attrsMoved_ = false;
        uint32_t sumW = 0;
        for (uint32_t w : r.words) sumW += w;
        static_assert(sizeof(AreasChange) == sizeof(ospf_areas_change), "records are the engine's");
        for (;;) {
          d.changes.resize(cap_);
          d.nh.resize((size_t)cap_ * sumW);
          d.rebased.resize(capReb_);
          uint32_t n = 0, nr = 0;
          rc = ospf_areastate_update(st_, sw.data(), r.words.data(),
                                     reinterpret_cast<ospf_areas_change*>(d.changes.data()),
                                     d.nh.data(), cap_, &n, d.rebased.data(), capReb_, &nr);
          if (rc == OSPF_E_RANGE && (n > cap_ || nr > capReb_)) {  // the lists did not fit: grow
            cap_ = std::max(cap_, n);
            capReb_ = std::max(capReb_, nr);
            continue;
          }
          d.changes.resize(rc == OSPF_OK ? n : 0);
          d.nh.resize(rc == OSPF_OK ? (size_t)n * sumW : 0);
          d.rebased.resize(rc == OSPF_OK ? nr : 0);
          break;
        }
        if (rc == OSPF_OK) {
          d.onDevice = true;
          remember(m, r);
          finish();
          return d;
        }
      }
      const std::string msg = ospf_areastate_last_error(st_);
      pull();  // the previous result off the device before any engine goes
      engineFailed(m, rc, msg);
    }
    pull();
    if (!hostOk_) {
      baseline();
      d = Delta{};
      d.words = words_;
      d.full = true;
      d.onDevice = st_ != nullptr;
      return d;
    }
  }
  AreasResult now = allAreasSelectImpl(given_, prefixes_, ulm_, AreasWhat::kHostOnly, &m);
  d.words = now.words;
  hostDiff(now, m, d);
  host_ = std::move(now);
  remember(m, host_);
  attrsMoved_ = false;
  finish();
  return d;
}

LinkState::AreasResult LinkState::AreasTracker::tracked(const std::vector<std::string>& nodes) {
  if (!st_ && !hostOk_) throw std::logic_error("AreasTracker::tracked: the baseline was lost (delta)");
  const size_t A = gid_.size(), P = prefixes_.size(), n = nodes.size();
  std::vector<uint32_t> ids;
  for (const auto& nm : nodes) {
    const auto it = std::lower_bound(names_.begin(), names_.end(), nm);
    if (it == names_.end() || *it != nm) throw std::invalid_argument("AreasTracker::tracked: unknown node " + nm);
    ids.push_back((uint32_t)(it - names_.begin()));
  }
  AreasResult r;
  r.order = order_;
  r.names = nodes;
  r.prefixes = (uint32_t)P;
  r.words = words_;
  for (auto* v : {&r.metric, &r.count, &r.links, &r.need, &r.best, &r.areas}) v->assign(n * P, 0);
  r.nh.resize(A);
  for (size_t a = 0; a < A; ++a) r.nh[a].assign(n * P * words_[a], 0);
  if (st_) {
    std::vector<uint32_t*> nhp;
    for (size_t a = 0; a < A; ++a) nhp.push_back(r.nh[a].data());
    const ospf_areas_pout o{r.metric.data(), r.count.data(), r.links.data(), r.need.data(),
                            r.best.data(),   r.areas.data(), nhp.data(),     words_.data()};
    if (const int rc = ospf_areastate_copy(st_, ids.data(), (uint32_t)n, &o))
      throw EngineError(rc, ospf_areastate_last_error(st_));
    r.onDevice = true;
  } else {
    for (size_t i = 0; i < n; ++i) {
      const uint32_t g = ids[i];
      for (auto [dst, src] : {std::pair{&r.metric, &host_.metric}, {&r.count, &host_.count},
                              {&r.links, &host_.links}, {&r.need, &host_.need},
                              {&r.best, &host_.best}, {&r.areas, &host_.areas}})
        std::copy(src->begin() + (size_t)g * P, src->begin() + (size_t)(g + 1) * P, dst->begin() + i * P);
      for (size_t a = 0; a < A; ++a) {
        const auto it = std::lower_bound(gid_[a].begin(), gid_[a].end(), g);
        if (it == gid_[a].end() || *it != g) continue;
        const size_t row = P * host_.words[a], la = it - gid_[a].begin();
        std::copy(host_.nh[a].begin() + la * row, host_.nh[a].begin() + (la + 1) * row,
                  r.nh[a].begin() + i * row);
      }
    }
  }
  markInstalled(r.links, r.need, r.installed);
  return r;
}

LinkState::PolicyResult LinkState::allSourcesSelect(
    const std::vector<std::vector<std::string>>& prefixes,
    const std::vector<std::vector<SelectAttr>>& attrs, bool useLinkMetric, uint32_t nhWords) {
  snapshot();
  const uint32_t W = wordsFor("allSourcesSelect", nhWords, selectWords(), kWidest);
  Lists ann, pref, mnh;
  policyTable(prefixes, attrs, "allSourcesSelect", ann, pref, mnh);
  return guarded([&] { return allSourcesPolicyImpl(ann, pref, mnh, useLinkMetric, W); });
}

LinkState::PolicyResult LinkState::allSourcesPolicyImpl(const Lists& ann, const Lists& pref,
                                                        const Lists& mnh, bool useLinkMetric,
                                                        uint32_t W) {
  snapshot();
  const size_t V = csr_->names.size(), P = ann.size();
  PolicyResult out = policyResult(V, P, W);
  if (!V || !P) return out;
  if (hostRun(useLinkMetric)) {
    // createRouteForPrefix's steps (SpfSolver.cpp:229-244, 649-676, 709-731,
    // 990-1000) over getSpfResult of every node
    BestClass b;
    for (uint32_t r = 0; r < V; ++r) {
      const SpfResult& res = getSpfResult(csr_->names[r], useLinkMetric);
      const LinkView links = linkView(*csr_, r, useLinkMetric);
      for (size_t p = 0; p < P; ++p) {
        if (!bestClass(res, *csr_, ann[p], pref[p], b)) continue;
        Metric shortest = std::numeric_limits<Metric>::max();
        for (size_t i : b.Sf) shortest = std::min(shortest, b.d[i]);
        const size_t cell = r * P + p;
        uint32_t* words = out.nh.data() + cell * W;
        for (size_t i : b.Sf) {
          out.need[cell] = std::max(out.need[cell], mnh[p][i]);
          if (b.d[i] != shortest) continue;
          ++out.count[cell];
          setNextHopBits(words, W, links.nbrs, csr_->ids, res.at(csr_->names[ann[p][i]]).nextHops());
        }
        out.metric[cell] = (uint32_t)shortest;
        out.best[cell] = bestOf(b.S, ann[p], r);
        out.links[cell] = linksOf(words, W, links.c);
      }
    }
    markInstalled(out.links, out.need, out.installed);
    return out;
  }
  prefetchAllSources(useLinkMetric);
  std::vector<uint32_t> off;
  const std::vector<uint32_t> nodes = flatten(ann, &off), prefs = flatten(pref), mins = flatten(mnh);
  const ospf_select_ptable t{(uint32_t)P, off.data(), nodes.data(), prefs.data(), mins.data()};
  if (msweep_) {
    const ospf_select_pout o = pout(out);
    const int rc = ospf_msweep_select_policy(msweep_, &t, W, &o);
    if (rc != OSPF_OK) throw EngineError(rc, ospf_multi_last_error(multi_));
  } else {
    const std::vector<uint32_t> roots = ownedRoots();
    PolicyResult own = policyResult(roots.size(), P, W);  // in owned-roots order
    const ospf_select_pout o = pout(own);
    const int rc = ospf_sweep_select_policy(sweep_, &t, W, &o);
    if (rc != OSPF_OK) throw EngineError(rc, ospf_sweep_last_error(sweep_));
    scatterOwned(roots, own.metric, out.metric, P);
    scatterOwned(roots, own.count, out.count, P);
    scatterOwned(roots, own.nh, out.nh, P * W);
    scatterOwned(roots, own.links, out.links, P);
    scatterOwned(roots, own.need, out.need, P);
    scatterOwned(roots, own.best, out.best, P);
  }
  markInstalled(out.links, out.need, out.installed);
  return out;
}

// ---------------------------------------------------------------- select SR_MPLS
LinkState::SrMplsResult LinkState::allSourcesSelectSrMpls(
    const std::vector<std::vector<std::string>>& prefixes,
    const std::vector<std::vector<SelectAttr>>& attrs,
    const std::vector<std::vector<uint8_t>>& hasPrepend, bool useLinkMetric, uint32_t nhWords) {
  snapshot();
  const uint32_t W = wordsFor("allSourcesSelectSrMpls", nhWords, selectWords(), kWidest);
  Lists ann, pref, mnh, pos, flags;
  policyTable(prefixes, attrs, "allSourcesSelectSrMpls", ann, pref, mnh, &pos);
  if (hasPrepend.size() != prefixes.size())
    throw std::invalid_argument("allSourcesSelectSrMpls: one prepend list per prefix");
  flags.resize(ann.size());
  for (size_t p = 0; p < ann.size(); ++p) {
    if (hasPrepend[p].size() != prefixes[p].size())
      throw std::invalid_argument("allSourcesSelectSrMpls: one prepend flag per announcer");
    for (uint32_t i : pos[p]) flags[p].push_back(hasPrepend[p][i] ? OSPF_SEL_SELF_PREPEND : 0u);
  }
  return guarded([&] { return allSourcesSrMplsImpl(ann, pref, mnh, flags, useLinkMetric, W); });
}

LinkState::SrMplsResult LinkState::allSourcesSrMplsImpl(const Lists& ann, const Lists& pref,
                                                        const Lists& mnh, const Lists& flags,
                                                        bool useLinkMetric, uint32_t W) {
  snapshot();
  const size_t V = csr_->names.size(), P = ann.size();
  SrMplsResult out;
  out.prefixes = (uint32_t)P;
  out.words = W;
  out.entryNodes = flatten(ann, &out.entryOffsets);
  const size_t A = out.entryNodes.size();
  out.metric.assign(V * P, kInf);
  out.best.assign(V * P, kInf);
  for (auto* v : {&out.count, &out.links, &out.need}) v->assign(V * P, 0);
  out.dstLinks.assign(V * A, 0);
  out.dstNh.assign(V * A * W, 0);
  out.installed.assign(V * P, 0);
  if (!V || !P) return out;
  // msweep has no SR_MPLS selection: a multi-device LinkState takes the host loop
  if (hostRun(useLinkMetric) || devices_.size() > 1) {
    // createRouteForPrefix's steps, then selectBestPathsSpf's per-destination
    // next hops (SpfSolver.cpp:794-806, 1043-1089) over getSpfResult of every node
    BestClass b;
    for (uint32_t r = 0; r < V; ++r) {
      const SpfResult& res = getSpfResult(csr_->names[r], useLinkMetric);
      const LinkView links = linkView(*csr_, r, useLinkMetric);
      for (size_t p = 0; p < P; ++p) {
        if (!bestClass(res, *csr_, ann[p], pref[p], b)) continue;
        const size_t cell = r * P + p;
        std::vector<size_t> D;
        for (size_t i : b.Sf) {
          out.need[cell] = std::max(out.need[cell], mnh[p][i]);
          // filteredBestNodeAreas: the node's own entry with a prepend label leaves
          if (!(ann[p][i] == r && (flags[p][i] & OSPF_SEL_SELF_PREPEND))) D.push_back(i);
        }
        out.best[cell] = bestOf(b.S, ann[p], r);
        if (D.empty()) continue;
        Metric shortest = std::numeric_limits<Metric>::max();
        for (size_t i : D) shortest = std::min(shortest, b.d[i]);
        out.metric[cell] = (uint32_t)shortest;
        for (size_t i : D) {
          if (b.d[i] != shortest) continue;
          ++out.count[cell];
          const size_t ent = r * A + out.entryOffsets[p] + i;
          setNextHopBits(out.dstNh.data() + ent * W, W, links.nbrs, csr_->ids,
                         res.at(csr_->names[ann[p][i]]).nextHops(),
                         [&](uint32_t k) { out.dstLinks[ent] += links.c[k]; });
          out.links[cell] += out.dstLinks[ent];
        }
      }
    }
    markInstalled(out.links, out.need, out.installed);
    return out;
  }
  prefetchAllSources(useLinkMetric);
  const std::vector<uint32_t> prefs = flatten(pref), mins = flatten(mnh), fl = flatten(flags);
  const ospf_select_stable t{(uint32_t)P,  out.entryOffsets.data(), out.entryNodes.data(),
                             prefs.data(), mins.data(),             fl.data()};
  const std::vector<uint32_t> roots = ownedRoots();
  const size_t n = roots.size();
  std::vector<uint32_t> m(n * P), k(n * P), li(n * P), ne(n * P), be(n * P), dl(n * A),
      dn(n * A * W);
  const ospf_select_sout o{m.data(), k.data(), li.data(), ne.data(), be.data(), dl.data(), dn.data()};
  const int rc = ospf_sweep_select_srmpls(sweep_, &t, W, &o);
  if (rc != OSPF_OK) throw EngineError(rc, ospf_sweep_last_error(sweep_));
  scatterOwned(roots, m, out.metric, P);
  scatterOwned(roots, k, out.count, P);
  scatterOwned(roots, li, out.links, P);
  scatterOwned(roots, ne, out.need, P);
  scatterOwned(roots, be, out.best, P);
  scatterOwned(roots, dl, out.dstLinks, A);
  scatterOwned(roots, dn, out.dstNh, A * W);
  markInstalled(out.links, out.need, out.installed);
  return out;
}

// ---------------------------------------------------------------- trackSelect
void LinkState::trackDropDev() {
  if (selstate_) ospf_selstate_destroy(selstate_);
  selstate_ = nullptr;
  trackDev_ = false;
  ucmpDev_ = false;
}

void LinkState::trackPull() {
  if (!trackDev_ || !selstate_) return;
  const size_t V = trackNames_.size(), P = trackPrefixes_.size();
  const uint32_t W = trackWords_;
  std::vector<uint32_t> ids(V);
  std::iota(ids.begin(), ids.end(), 0u);
  int rc;
  if (trackPolicy_) {
    PolicyResult r = policyResult(V, P, W);
    const ospf_select_pout o = pout(r);
    rc = ospf_selstate_copy_policy(selstate_, ids.data(), (uint32_t)V, W, &o);
    markInstalled(r.links, r.need, r.installed);
    if (rc == OSPF_OK) trackHostP_ = std::move(r);
  } else {
    SelectResult r = selectResult(V, P, W);
    rc = ospf_selstate_copy(selstate_, ids.data(), (uint32_t)V, W, r.metric.data(), r.count.data(),
                            r.nh.data());
    if (rc == OSPF_OK) trackHost_ = std::move(r);
  }
  trackDev_ = false;
  trackHostOk_ = rc == OSPF_OK;
}

void LinkState::trackPrime() {
  snapshot();
  const size_t V = csr_->names.size();
  const auto ann = trackAnn();
  trackDropDev();
  trackHostOk_ = false;
  trackHost_ = SelectResult{};
  trackHostP_ = PolicyResult{};
  trackAttrsMoved_ = false;
  const uint32_t W = selectWords();
  Lists pann, pref, mnh;
  if (trackPolicy_) policyTable(trackPrefixes_, trackAttrs_, "trackSelect", pann, pref, mnh);
  if (!hostRun(trackMetric_) && devices_.size() == 1 && V) {
    prefetchAllSources(trackMetric_);
    std::vector<uint32_t> off;
    const std::vector<uint32_t> nodes = flatten(ann, &off), prefs = flatten(pref), mins = flatten(mnh);
    const ospf_select_table t{(uint32_t)ann.size(), off.data(), nodes.data()};
    const ospf_select_ptable pt{t.n_prefixes, off.data(), nodes.data(), prefs.data(), mins.data()};
    int rc = trackPolicy_ ? ospf_selstate_create_policy(engine_, &pt, &selstate_)
                          : ospf_selstate_create(engine_, &t, &selstate_);
    if (rc != OSPF_OK) throw EngineError(rc, ospf_last_error(engine_));
    rc = ospf_selstate_prime(selstate_, sweep_);
    if (rc != OSPF_OK) {
      const std::string m = ospf_selstate_last_error(selstate_);
      trackDropDev();
      throw EngineError(rc, m);
    }
    trackDev_ = true;
  } else {
    if (trackPolicy_) trackHostP_ = allSourcesPolicyImpl(ann, pref, mnh, trackMetric_, W);
    else trackHost_ = allSourcesSelectImpl(ann, trackMetric_, W);
    trackHostOk_ = true;
  }
  trackNames_ = csr_->names;
  trackWords_ = W;
  trackNbrs_.resize(V);
  for (uint32_t v = 0; v < V; ++v) trackNbrs_[v] = nbrsOf(v);
  trackVersion_ = snapVersion_;
}

void LinkState::trackSelect(const std::vector<std::vector<std::string>>& prefixes,
                            bool useLinkMetric) {
  trackPrefixes_ = prefixes;
  trackAttrs_.clear();
  trackPolicy_ = false;
  trackMetric_ = useLinkMetric;
  tracking_ = true;
  guarded([&] { trackPrime(); });
}

void LinkState::trackSelect(const std::vector<std::vector<std::string>>& prefixes,
                            const std::vector<std::vector<SelectAttr>>& attrs, bool useLinkMetric) {
  snapshot();
  Lists ann, pref, mnh;
  policyTable(prefixes, attrs, "trackSelect", ann, pref, mnh);  // the argument checks
  trackPrefixes_ = prefixes;
  trackAttrs_ = attrs;
  trackPolicy_ = true;
  trackMetric_ = useLinkMetric;
  tracking_ = true;
  guarded([&] { trackPrime(); });
}

void LinkState::setTrackedAttrs(const std::vector<std::vector<SelectAttr>>& attrs) {
  if (!tracking_ || !trackPolicy_)
    throw std::logic_error("setTrackedAttrs: no table tracked with attributes (trackSelect)");
  snapshot();
  Lists ann, pref, mnh;
  policyTable(trackPrefixes_, attrs, "setTrackedAttrs", ann, pref, mnh);
  trackAttrs_ = attrs;
  trackAttrsMoved_ = true;
  ucmpDev_ = ucmpHostOk_ = false;
  // the device state's columns are replaced by the next policyDelta, once it
  // knows that the state's table is still the snapshot's (trackAttrsMoved_)
}

// What selectDelta and policyDelta differ in: the records, the engine's update
// call, the host recompute and the scalar columns compared
struct LinkState::PlainTrack {
  using Delta = SelectDelta;
  using Result = SelectResult;
  using Rec = ospf_select_change;
  static constexpr auto update = ospf_selstate_update;
  static Result& host(LinkState& ls) { return ls.trackHost_; }
  static Result recompute(LinkState& ls, uint32_t W) {
    return ls.allSourcesSelectImpl(ls.trackAnn(), ls.trackMetric_, W);
  }
  static bool differ(const Result& a, const Result& b, size_t i) {
    return a.metric[i] != b.metric[i] || a.count[i] != b.count[i];
  }
  static SelectChange change(const Rec& r) { return {r.root, r.prefix, r.metric, r.count}; }
  static SelectChange change(uint32_t v, uint32_t p, const Result& n, size_t i) {
    return {v, p, n.metric[i], n.count[i]};
  }
};
struct LinkState::PolicyTrack {
  using Delta = PolicyDelta;
  using Result = PolicyResult;
  using Rec = ospf_select_pchange;
  static constexpr auto update = ospf_selstate_update_policy;
  static Result& host(LinkState& ls) { return ls.trackHostP_; }
  static Result recompute(LinkState& ls, uint32_t W) {
    Lists ann, pref, mnh;
    ls.policyTable(ls.trackPrefixes_, ls.trackAttrs_, "policyDelta", ann, pref, mnh);
    return ls.allSourcesPolicyImpl(ann, pref, mnh, ls.trackMetric_, W);
  }
  static bool differ(const Result& a, const Result& b, size_t i) {
    return a.metric[i] != b.metric[i] || a.count[i] != b.count[i] || a.links[i] != b.links[i] ||
           a.need[i] != b.need[i] || a.best[i] != b.best[i];
  }
  static PolicyChange change(const Rec& r) {
    return {r.root, r.prefix, r.metric, r.count, r.links, r.need, r.best, r.installed};
  }
  static PolicyChange change(uint32_t v, uint32_t p, const Result& n, size_t i) {
    return {v, p, n.metric[i], n.count[i], n.links[i], n.need[i], n.best[i], n.installed[i]};
  }
};

template <class T>
typename T::Delta LinkState::trackedDelta() {
  snapshot();
  typename T::Delta out;
  const size_t V = csr_->names.size(), P = trackPrefixes_.size();
  const uint32_t W = selectWords();
  out.words = W;
  const auto anew = [&] {
    trackPrime();
    out.full = true;
    return out;
  };
  // the ids were renumbered, or no baseline survived (a device error that
  // took it along): everything anew
  if (csr_->names != trackNames_ || (!trackDev_ && !trackHostOk_)) return anew();
  const bool dev = !hostRun(trackMetric_) && devices_.size() == 1;
  if (dev && trackDev_) {
    prefetchAllSources(trackMetric_);  // re-sweeps when the version moved
    if (trackPolicy_ && trackAttrsMoved_) {  // setTrackedAttrs since the last delta
      // the node names are the tracked ones here, so the ids are the state's
      Lists ann, pref, mnh;
      policyTable(trackPrefixes_, trackAttrs_, "policyDelta", ann, pref, mnh);
      const std::vector<uint32_t> prefs = flatten(pref), mins = flatten(mnh);
      const int rc = ospf_selstate_set_policy(selstate_, prefs.data(), mins.data());
      if (rc != OSPF_OK) throw EngineError(rc, ospf_selstate_last_error(selstate_));
    }
    uint32_t cap = 1024, capReb = 64, n = 0, nReb = 0;
    std::vector<typename T::Rec> recs;
    for (;;) {
      recs.resize(cap);
      out.nh.assign((size_t)cap * W, 0);
      out.rebased.assign(capReb, 0);
      const int rc = T::update(selstate_, sweep_, W, recs.data(), out.nh.data(), cap, &n,
                               out.rebased.data(), capReb, &nReb);
      if (rc == OSPF_OK) break;
      if (rc != OSPF_E_RANGE) throw EngineError(rc, ospf_selstate_last_error(selstate_));
      cap = std::max(cap, n);  // the state is unchanged: the same call, large enough
      capReb = std::max(capReb, nReb);
    }
    for (uint32_t i = 0; i < n; ++i) out.changes.push_back(T::change(recs[i]));
    out.nh.resize((size_t)n * W);
    out.rebased.resize(nReb);
    std::sort(out.rebased.begin(), out.rebased.end());
  } else {
    if (trackDev_) trackPull();  // the host takes over with the device's baseline
    if (!trackHostOk_) return anew();
    trackDropDev();
    typename T::Result now = T::recompute(*this, W);
    const typename T::Result& was = T::host(*this);
    for (uint32_t v = 0; v < V; ++v) {
      if (nbrsOf(v) != trackNbrs_[v]) {
        out.rebased.push_back(v);
        continue;
      }
      for (size_t p = 0; p < P; ++p) {
        const size_t i = v * P + p;
        bool ch = T::differ(now, was, i);
        for (uint32_t w = 0; w < std::max(W, was.words) && !ch; ++w)
          ch = (w < W ? now.nh[i * W + w] : 0u) != (w < was.words ? was.nh[i * was.words + w] : 0u);
        if (!ch) continue;
        out.changes.push_back(T::change(v, (uint32_t)p, now, i));
        out.nh.insert(out.nh.end(), now.nh.begin() + i * W, now.nh.begin() + (i + 1) * W);
      }
    }
    T::host(*this) = std::move(now);
  }
  trackWords_ = W;
  for (uint32_t v : out.rebased) trackNbrs_[v] = nbrsOf(v);
  trackVersion_ = snapVersion_;
  trackAttrsMoved_ = false;
  return out;
}

LinkState::PolicyDelta LinkState::policyDelta() {
  if (!tracking_ || !trackPolicy_)
    throw std::logic_error("policyDelta: no table tracked with attributes (trackSelect)");
  return guarded([&] { return trackedDelta<PolicyTrack>(); });
}

LinkState::PolicyResult LinkState::policyTracked(const std::vector<std::string>& nodes,
                                                 uint32_t nhWords) {
  if (!tracking_ || !trackPolicy_)
    throw std::logic_error("policyTracked: no table tracked with attributes (trackSelect)");
  if (!trackDev_ && !trackHostOk_) throw std::logic_error("policyTracked: no baseline (policyDelta)");
  const uint32_t W = wordsFor("policyTracked", nhWords, trackWords_, kBaseline);
  const auto ids = trackIds(nodes, "policyTracked");
  return guarded([&] {
    const size_t P = trackPrefixes_.size();
    PolicyResult r = policyResult(ids.size(), P, W);
    if (trackDev_) {
      const ospf_select_pout o = pout(r);
      const int rc = ospf_selstate_copy_policy(selstate_, ids.data(), (uint32_t)ids.size(), W, &o);
      if (rc != OSPF_OK) throw EngineError(rc, ospf_selstate_last_error(selstate_));
    } else {
      if (!trackHostOk_) throw std::logic_error("policyTracked: the baseline was lost (policyDelta)");
      const PolicyResult& h = trackHostP_;
      gatherRows(ids, P, h.metric, 1, r.metric, 1);
      gatherRows(ids, P, h.count, 1, r.count, 1);
      gatherRows(ids, P, h.links, 1, r.links, 1);
      gatherRows(ids, P, h.need, 1, r.need, 1);
      gatherRows(ids, P, h.best, 1, r.best, 1);
      gatherRows(ids, P, h.nh, h.words, r.nh, W);
    }
    markInstalled(r.links, r.need, r.installed);
    return r;
  });
}

LinkState::SelectDelta LinkState::selectDelta() {
  if (!tracking_) throw std::logic_error("selectDelta: no tracked table (trackSelect)");
  if (trackPolicy_) throw std::logic_error("selectDelta: the table is tracked with attributes (policyDelta)");
  return guarded([&] { return trackedDelta<PlainTrack>(); });
}

LinkState::SelectResult LinkState::selectTracked(const std::vector<std::string>& nodes,
                                                 uint32_t nhWords) {
  if (!tracking_) throw std::logic_error("selectTracked: no tracked table (trackSelect)");
  if (trackPolicy_)
    throw std::logic_error("selectTracked: the table is tracked with attributes (policyTracked)");
  if (!trackDev_ && !trackHostOk_) throw std::logic_error("selectTracked: no baseline (selectDelta)");
  const uint32_t W = wordsFor("selectTracked", nhWords, trackWords_, kBaseline);
  const auto ids = trackIds(nodes, "selectTracked");
  return guarded([&] {
    const size_t P = trackPrefixes_.size();
    SelectResult r = selectResult(ids.size(), P, W);
    if (trackDev_) {
      const int rc = ospf_selstate_copy(selstate_, ids.data(), (uint32_t)ids.size(), W,
                                        r.metric.data(), r.count.data(), r.nh.data());
      if (rc != OSPF_OK) throw EngineError(rc, ospf_selstate_last_error(selstate_));
      return r;
    }
    if (!trackHostOk_) throw std::logic_error("selectTracked: the baseline was lost (selectDelta)");
    const SelectResult& h = trackHost_;
    gatherRows(ids, P, h.metric, 1, r.metric, 1);
    gatherRows(ids, P, h.count, 1, r.count, 1);
    gatherRows(ids, P, h.nh, h.words, r.nh, W);
    return r;
  });
}

// ---------------------------------------------------------------- allSourcesUcmp
void LinkState::trackCurrent(const char* who) {
  if (!tracking_) throw std::logic_error(std::string(who) + ": no tracked table (trackSelect)");
  snapshot();
  if (snapVersion_ != trackVersion_ || csr_->names != trackNames_ || (!trackDev_ && !trackHostOk_) ||
      trackAttrsMoved_)
    throw std::logic_error(std::string(who) + ": the tracked selection is older than the topology" +
                           " or its attributes (selectDelta / policyDelta)");
}

std::vector<std::vector<int64_t>> LinkState::trackLeafWeights(
    const std::vector<std::vector<uint32_t>>& ann,
    const std::vector<std::vector<int64_t>>& leafWeights) const {
  if (leafWeights.size() != trackPrefixes_.size())
    throw std::invalid_argument("allSourcesUcmp: one weight list per tracked prefix");
  std::vector<std::vector<int64_t>> out(ann.size());
  for (size_t p = 0; p < ann.size(); ++p) {
    if (leafWeights[p].size() != trackPrefixes_[p].size())
      throw std::invalid_argument("allSourcesUcmp: one weight per announcer name of prefix " +
                                  std::to_string(p));
    std::unordered_map<uint32_t, int64_t> by;  // the first weight given for an id
    for (size_t i = 0; i < trackPrefixes_[p].size(); ++i) {
      if (leafWeights[p][i] < 0) throw std::invalid_argument("allSourcesUcmp: a negative weight");
      const auto it = csr_->ids.find(trackPrefixes_[p][i]);
      if (it != csr_->ids.end()) by.emplace(it->second, leafWeights[p][i]);
    }
    for (uint32_t a : ann[p]) out[p].push_back(by.at(a));
  }
  return out;
}

std::vector<uint32_t> LinkState::trackIds(const std::vector<std::string>& nodes, const char* who) const {
  std::vector<uint32_t> ids;
  for (const auto& nm : nodes) {
    const auto it = std::lower_bound(trackNames_.begin(), trackNames_.end(), nm);
    if (it == trackNames_.end() || *it != nm)
      throw std::invalid_argument(std::string(who) + ": unknown node " + nm);
    ids.push_back((uint32_t)(it - trackNames_.begin()));
  }
  return ids;
}

LinkState::UcmpView LinkState::ucmpHostImpl(UcmpAlgo algo, const std::vector<std::vector<uint32_t>>& ann,
                                            const std::vector<std::vector<int64_t>>& w,
                                            const std::vector<uint32_t>& ids) {
  const size_t P = ann.size();
  std::vector<std::vector<uint32_t>> pann, pref, mnh;  // a policy table: its class ranks
  if (trackPolicy_) {
    policyTable(trackPrefixes_, trackAttrs_, "allSourcesUcmp", pann, pref, mnh);
    if (pann != ann) throw std::logic_error("allSourcesUcmp: the class ranks are not the table's");
  }
  UcmpView out;
  out.prefixes = (uint32_t)P;
  out.weight.assign(ids.size() * P, 0);
  out.status.assign(ids.size() * P, OSPF_UCMP_NONE);
  out.off.assign(ids.size() * P + 1, 0);
  for (size_t i = 0; i < ids.size(); ++i) {
    const std::string& me = csr_->names[ids[i]];
    const SpfResult& res = getSpfResult(me, trackMetric_);
    const std::vector<uint32_t> nbrs = nbrsOf(ids[i]);
    for (size_t p = 0; p < P; ++p) {
      const size_t e = i * P + p;
      out.off[e + 1] = out.wt.size();
      // the min-cost announcers (getNextHopsWithMetric) and their weights
      Metric shortest = std::numeric_limits<Metric>::max();
      std::unordered_map<std::string, int64_t> leaves;
      bool zero = false;
      // under the policy the walk starts from its filtered set: the reached
      // announcers of the best class, the drained ones dropped unless all are
      uint32_t top = kInf;
      bool undrained = false;
      if (trackPolicy_) {
        for (size_t k = 0; k < ann[p].size(); ++k)
          if (res.find(csr_->names[ann[p][k]]) != res.end()) top = std::min(top, pref[p][k]);
        for (size_t k = 0; k < ann[p].size(); ++k)
          undrained |= pref[p][k] == top && !csr_->noTransit[ann[p][k]] &&
                       res.find(csr_->names[ann[p][k]]) != res.end();
      }
      for (size_t k = 0; k < ann[p].size(); ++k) {
        const auto it = res.find(csr_->names[ann[p][k]]);
        if (it == res.end()) continue;
        if (trackPolicy_ && (pref[p][k] != top || (undrained && csr_->noTransit[ann[p][k]]))) continue;
        const Metric d = it->second.metric();
        if (d > shortest) continue;
        if (d < shortest) {
          shortest = d;
          leaves.clear();
          zero = false;
        }
        leaves.emplace(csr_->names[ann[p][k]], w[p][k]);
        zero |= w[p][k] == 0;
      }
      if (leaves.empty()) continue;
      if (zero) {  // getNodeUcmpResult returns nullopt (SpfSolver.cpp:1139-1142)
        out.status[e] = OSPF_UCMP_VOID;
        continue;
      }
      const UcmpResult all = resolveUcmpWeights(res, leaves, algo, trackMetric_);
      const auto mine = all.find(me);
      if (mine == all.end()) continue;
      out.status[e] = OSPF_UCMP_OK;
      out.weight[e] = mine->second.weight().value_or(0);
      std::map<uint32_t, int64_t> byNbr;  // every tight link to a neighbour carries its weight
      for (const auto& kv : mine->second.nextHopLinks())
        byNbr.emplace(csr_->ids.at(kv.second.nextHopNode), kv.second.weight);
      for (uint32_t k : nbrs) {
        const auto it = byNbr.find(k);
        if (it != byNbr.end()) out.wt.push_back(it->second);
      }
      out.off[e + 1] = out.wt.size();
    }
  }
  return out;
}

LinkState::UcmpAll LinkState::allSourcesUcmp(UcmpAlgo algo,
                                             const std::vector<std::vector<int64_t>>& leafWeights) {
  if (algo != UcmpAlgo::kAdjWeightPropagation && algo != UcmpAlgo::kPrefixWeightPropagation)
    throw std::invalid_argument("allSourcesUcmp: not a UCMP algorithm");
  trackCurrent("allSourcesUcmp");
  const auto ann = trackAnn();
  const auto w = trackLeafWeights(ann, leafWeights);
  return guarded([&] {
    const size_t V = csr_->names.size(), P = ann.size();
    UcmpAll out;
    out.prefixes = (uint32_t)P;
    ucmpDev_ = ucmpHostOk_ = false;
    // S per (node, distinct neighbour): the node's link weights over the
    // tight links (up, at the smallest metric towards the neighbour; every
    // up link under hop count), slots in nbrsOf order, node after node.
    // False when a link weight is negative or a slot's sum leaves i63: the
    // engine takes sums in [0, 2^63 - 1] only, so that call is the host
    // loop's, as with a metric outside the engine contract.
    std::vector<int64_t> S;
    const auto linkSums = [&] {
      for (uint32_t u = 0; u < V; ++u) {
        uint32_t e = csr_->rowPtr[u];
        const uint32_t hi = csr_->rowPtr[u + 1];
        while (e < hi) {
          const uint32_t k = csr_->col[e];
          uint32_t best = std::numeric_limits<uint32_t>::max();
          int64_t sum = 0;
          for (; e < hi && csr_->col[e] == k; ++e) {
            if (!csr_->edgeUp[e]) continue;
            const uint32_t m = trackMetric_ ? csr_->metric[e] : 1u;
            if (m > best) continue;
            if (m < best) {
              best = m;
              sum = 0;
            }
            const int64_t lw = csr_->links.at(csr_->linkId[e])->weightFrom(csr_->names[u]);
            if (lw < 0 || __builtin_add_overflow(sum, lw, &sum)) return false;
          }
          if (k != u) S.push_back(sum);
        }
      }
      return true;
    };
    if (trackDev_ && !hostRun(trackMetric_) && devices_.size() == 1 && linkSums()) {
      std::vector<int64_t> flat;
      for (const auto& l : w) flat.insert(flat.end(), l.begin(), l.end());
      const auto t0 = std::chrono::steady_clock::now();
      const int rc = ospf_selstate_ucmp(selstate_, (uint32_t)algo, flat.data(), S.data(),
                                        (uint32_t)S.size(), &out.rounds);
      out.engineMs =
          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (rc != OSPF_OK) throw EngineError(rc, ospf_selstate_last_error(selstate_));
      out.weight.assign(V * P, 0);
      out.status.assign(V * P, OSPF_UCMP_NONE);
      std::vector<uint32_t> ids(V);
      for (uint32_t v = 0; v < V; ++v) ids[v] = v;
      uint64_t n = 0;
      const int rc2 = ospf_selstate_ucmp_copy(selstate_, ids.data(), (uint32_t)V, out.weight.data(),
                                              out.status.data(), nullptr, nullptr, 0, &n);
      if (rc2 != OSPF_OK) throw EngineError(rc2, ospf_selstate_last_error(selstate_));
      out.device = true;
      ucmpDev_ = true;
    } else {
      std::vector<uint32_t> ids(V);
      for (uint32_t v = 0; v < V; ++v) ids[v] = v;
      ucmpHost_ = ucmpHostImpl(algo, ann, w, ids);
      ucmpHostOk_ = true;
      out.weight = ucmpHost_.weight;
      out.status = ucmpHost_.status;
    }
    ucmpVersion_ = trackVersion_;
    return out;
  });
}

LinkState::UcmpView LinkState::ucmpHostLoop(UcmpAlgo algo,
                                            const std::vector<std::vector<int64_t>>& leafWeights,
                                            const std::vector<std::string>& nodes) {
  trackCurrent("ucmpHostLoop");
  const auto ann = trackAnn();
  const auto w = trackLeafWeights(ann, leafWeights);
  const auto ids = trackIds(nodes, "ucmpHostLoop");
  return guarded([&] { return ucmpHostImpl(algo, ann, w, ids); });
}

LinkState::UcmpView LinkState::ucmpTracked(const std::vector<std::string>& nodes) {
  trackCurrent("ucmpTracked");
  if ((!ucmpDev_ && !ucmpHostOk_) || ucmpVersion_ != trackVersion_)
    throw std::logic_error("ucmpTracked: no UCMP result of the tracked selection (allSourcesUcmp)");
  const auto ids = trackIds(nodes, "ucmpTracked");
  const size_t n = ids.size(), P = trackPrefixes_.size();
  UcmpView r;
  r.prefixes = (uint32_t)P;
  r.weight.assign(n * P, 0);
  r.status.assign(n * P, OSPF_UCMP_NONE);
  r.off.assign(n * P + 1, 0);
  if (ucmpDev_) {
    // a device error here is not degraded: the result lives on the device
    // only, so the caller resolves again (allSourcesUcmp, which degrades)
    uint64_t need = 0;
    for (uint64_t cap = 1024;;) {
      r.wt.assign(cap, 0);
      const int rc = ospf_selstate_ucmp_copy(selstate_, ids.data(), (uint32_t)n, r.weight.data(),
                                             r.status.data(), r.off.data(), r.wt.data(), cap, &need);
      if (rc == OSPF_OK) break;
      if (rc != OSPF_E_RANGE) throw EngineError(rc, ospf_selstate_last_error(selstate_));
      cap = need;  // nothing was written: the same call, large enough
    }
    r.wt.resize(need);
    return r;
  }
  const UcmpView& h = ucmpHost_;
  for (size_t i = 0; i < n; ++i)
    for (size_t p = 0; p < P; ++p) {
      const size_t s = (size_t)ids[i] * P + p;
      r.weight[i * P + p] = h.weight[s];
      r.status[i * P + p] = h.status[s];
      r.wt.insert(r.wt.end(), h.wt.begin() + h.off[s], h.wt.begin() + h.off[s + 1]);
      r.off[i * P + p + 1] = r.wt.size();
    }
  return r;
}

void LinkState::evictSpf(const std::vector<std::string>& roots, bool useLinkMetric) {
  auto& memo = useLinkMetric ? memoMetric_ : memoHops_;
  for (const auto& r : roots) memo.erase(r);
}

uint32_t LinkState::nhWordsFor(uint32_t root) const {
  uint32_t n = 0;
  for (uint32_t e = csr_->rowPtr[root]; e < csr_->rowPtr[root + 1]; ++e)
    if (csr_->col[e] != root && (e == csr_->rowPtr[root] || csr_->col[e - 1] != csr_->col[e])) ++n;
  return std::max<uint32_t>(1, (n + 31) / 32);
}

std::vector<ospf_ctx*> LinkState::slots() const {
  std::vector<ospf_ctx*> out;
  if (multi_) {
    for (uint32_t i = 0, n = ospf_multi_size(multi_); i < n; ++i) out.push_back(ospf_multi_ctx(multi_, i));
  } else if (engine_) {
    out.push_back(engine_);
  }
  return out;
}

int LinkState::batchOn(ospf_ctx* c, const uint32_t* roots, uint32_t n, bool useLinkMetric,
                       uint32_t flags, uint32_t W, uint32_t* dist, uint32_t* nh) const {
  if (!useLinkMetric) flags |= OSPF_HOP_COUNT;
  return ospf_sssp_batch(c, roots, n, nullptr, flags, W, dist, nh, nullptr);
}

// Run fn(slot, ctx) for every slot, slot 0 on the calling thread; the first
// failure (rc, slot) is returned after every thread joined. A slot whose
// thread cannot be created runs on the calling thread too.
static std::pair<int, size_t> onSlots(const std::vector<ospf_ctx*>& cs,
                                      const std::function<int(size_t, ospf_ctx*)>& fn) {
  std::vector<int> rc(cs.size(), OSPF_OK);
  std::vector<std::thread> th;
  std::vector<size_t> here{0};
  for (size_t i = 1; i < cs.size(); ++i) {
    try {
      th.emplace_back([&, i] { rc[i] = fn(i, cs[i]); });
    } catch (const std::system_error&) {
      here.push_back(i);
    }
  }
  for (size_t i : here) rc[i] = fn(i, cs[i]);
  for (auto& t : th) t.join();
  for (size_t i = 0; i < cs.size(); ++i)
    if (rc[i] != OSPF_OK) return {rc[i], i};
  return {OSPF_OK, 0};
}

void LinkState::runBatch(const std::vector<uint32_t>& roots,
                         const std::vector<std::vector<uint32_t>>* ign, bool useLinkMetric,
                         uint32_t flags, uint32_t W, std::vector<uint32_t>* dist,
                         std::vector<uint32_t>* nh, std::vector<ospf_digest>* dig) {
  ensureEngine();
  const size_t V = csr_->names.size(), n = roots.size();
  if (!useLinkMetric) flags |= OSPF_HOP_COUNT;
  if (dist) dist->assign(n * V, kInf);
  if (nh) nh->assign(n * V * W, 0);
  if (dig) dig->assign(n, ospf_digest{0, 0, 0});
  std::vector<uint32_t> off, ids;
  ospf_ignore ig{};
  if (ign) {
    off.reserve(n + 1);
    off.push_back(0);
    for (const auto& l : *ign) {
      ids.insert(ids.end(), l.begin(), l.end());
      off.push_back((uint32_t)ids.size());
    }
    ig.offsets = off.data();
    ig.link_ids = ids.data();
  }
  int rc = ospf_sssp_batch(engine_, roots.data(), (uint32_t)n, ign ? &ig : nullptr, flags, W,
                           dist ? dist->data() : nullptr, nh ? nh->data() : nullptr,
                           dig ? dig->data() : nullptr);
  if (rc != OSPF_OK) throw EngineError(rc, ospf_last_error(engine_));
}

// ---------------------------------------------------------------- results
std::vector<PathLink> SpfRows::pathLinksOf(uint32_t v) const {
  std::vector<PathLink> out;
  const CsrSnapshot& c = *csr;
  const uint32_t dv = dist[v];
  if (v == root || dv == kInf) return out;
  struct Cand {
    uint32_t du, u, rank, lid;
  };
  std::vector<Cand> cands;
  for (uint32_t e = c.rowPtr[v]; e < c.rowPtr[v + 1]; ++e) {
    if (!c.edgeUp[e]) continue;
    const uint32_t lid = c.linkId[e];
    if (!ignored.empty() && std::binary_search(ignored.begin(), ignored.end(), lid)) continue;
    const uint32_t u = c.col[e];
    const uint32_t du = dist[u];
    if (du == kInf) continue;
    const uint32_t t = c.twin[e];  // entry u -> v: metric advertised by u
    const uint64_t w = useLinkMetric ? c.metric[t] : 1u;
    if ((uint64_t)du + w != dv) continue;
    if (u != root && c.noTransit[u]) continue;
    cands.push_back({du, u, c.linkRank[t], lid});
  }
  // reference order: predecessor pop order (dist, name) then the link's
  // position in linksFromNode(predecessor)
  std::sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) {
    return std::tie(a.du, a.u, a.rank) < std::tie(b.du, b.u, b.rank);
  });
  out.reserve(cands.size());
  for (const auto& x : cands) out.push_back(PathLink{c.links[x.lid], c.names[x.u]});
  return out;
}

std::unordered_set<std::string> SpfRows::nextHopsOf(uint32_t v) const {
  std::unordered_set<std::string> out;
  if (nh.empty()) return out;
  const uint32_t* bits = nh.data() + (size_t)v * W;
  for (uint32_t w = 0; w < W; ++w)
    for (uint32_t b = bits[w]; b; b &= b - 1) {
      const uint32_t i = w * 32 + (uint32_t)__builtin_ctz(b);
      out.insert(csr->names[nbrs.at(i)]);
    }
  return out;
}

SpfResult::SpfResult(std::shared_ptr<const SpfRows> rows) : rows_(std::move(rows)) {
  const auto& d = rows_->dist;
  size_t n = 0;
  for (const uint32_t x : d) n += x != kInf;
  reached_.reserve(n);
  for (uint32_t v = 0; v < (uint32_t)d.size(); ++v)
    if (d[v] != kInf) reached_.push_back(v);
  slot_ = std::make_unique<std::atomic<value_type*>[]>(n);  // value-initialised: null
}

SpfResult::SpfResult(SpfResult&& o) noexcept
    : map_(std::move(o.map_)), rows_(std::move(o.rows_)), reached_(std::move(o.reached_)),
      slot_(std::move(o.slot_)) {
  o.reached_.clear();
}

SpfResult& SpfResult::operator=(SpfResult&& o) noexcept {
  if (this != &o) {
    release();
    map_ = std::move(o.map_);
    rows_ = std::move(o.rows_);
    reached_ = std::move(o.reached_);
    slot_ = std::move(o.slot_);
    o.reached_.clear();
  }
  return *this;
}

void SpfResult::release() {
  if (slot_)
    for (size_t k = 0; k < reached_.size(); ++k) delete slot_[k].load(std::memory_order_relaxed);
  slot_.reset();
}

const SpfResult::value_type& SpfResult::entry(size_t k) const {
  value_type* p = slot_[k].load(std::memory_order_acquire);
  if (p) return *p;
  const uint32_t v = reached_[k];
  auto* fresh = new value_type(std::piecewise_construct, std::forward_as_tuple(rows_->csr->names[v]),
                               std::forward_as_tuple(NodeSpfResult(rows_->dist[v], rows_.get(), v)));
  if (slot_[k].compare_exchange_strong(p, fresh, std::memory_order_acq_rel)) return *fresh;
  delete fresh;  // another thread made it first
  return *p;
}

SpfResult::const_iterator SpfResult::begin() const {
  const_iterator it;
  it.r_ = this;
  if (!rows_) it.m_ = map_.begin();
  return it;
}

SpfResult::const_iterator SpfResult::end() const {
  const_iterator it;
  it.r_ = this;
  if (rows_) it.k_ = reached_.size();
  else it.m_ = map_.end();
  return it;
}

SpfResult::const_iterator SpfResult::find(const std::string& node) const {
  if (!rows_) {
    const_iterator it;
    it.r_ = this;
    it.m_ = map_.find(node);
    return it;
  }
  const auto& ids = rows_->csr->ids;
  auto id = ids.find(node);
  if (id == ids.end() || rows_->dist[id->second] == kInf) return end();
  const_iterator it;
  it.r_ = this;
  it.k_ = (size_t)(std::lower_bound(reached_.begin(), reached_.end(), id->second) - reached_.begin());
  return it;
}

const NodeSpfResult& SpfResult::at(const std::string& node) const {
  auto it = find(node);
  if (it == end()) throw std::out_of_range("SpfResult::at: " + node);
  return it->second;
}

std::vector<uint32_t> LinkState::nbrsOf(uint32_t root) const { return distinctNbrs(*csr_, root); }

const SpfResult& LinkState::getSpfResultImpl(const std::string& node, bool useLinkMetric) {
  auto& memo = useLinkMetric ? memoMetric_ : memoHops_;
  auto it = memo.find(node);
  if (it != memo.end()) return it->second;
  prefetchSpf({node}, useLinkMetric);
  return memo.at(node);
}

void LinkState::prefetchSpfImpl(const std::vector<std::string>& roots, bool useLinkMetric) {
  auto& memo = useLinkMetric ? memoMetric_ : memoHops_;
  snapshot();
  std::unordered_map<uint32_t, std::vector<uint32_t>> byW;  // W -> roots
  std::unordered_set<std::string> queued;
  size_t pending = 0;
  for (const auto& r : roots) {
    if (memo.count(r) || !queued.insert(r).second) continue;
    auto id = csr_->ids.find(r);
    if (id == csr_->ids.end()) {  // no adjacency DB: only the root itself
      ++spfRuns_;
      SpfResult::Map res;
      res.emplace(r, NodeSpfResult(0));
      memo.emplace(r, SpfResult(std::move(res)));
      continue;
    }
    if (hostRun(useLinkMetric)) {
      ++spfRuns_;
      memo.emplace(r, runSpfHost(r, useLinkMetric, {}));
      continue;
    }
    byW[nhWordsFor(id->second)].push_back(id->second);
    ++pending;
  }
  const size_t V = csr_->names.size();
  // most of the nodes asked for: one all-sources sweep, rows copied from it
  if (!sweepHas(useLinkMetric) && pending >= kSweepMinRoots && 2 * pending >= V)
    prefetchAllSources(useLinkMetric);
  const bool fromSweep = sweepHas(useLinkMetric);
  if (!fromSweep) spfRuns_ += pending;  // a sweep counted every node's run
  for (auto& [W, ids] : byW) {
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(ids.size(), (256ull << 20) / (V * 4 * (1 + W))));
    for (size_t c0 = 0; c0 < ids.size(); c0 += chunk) {
      std::vector<uint32_t> part(ids.begin() + c0, ids.begin() + std::min(ids.size(), c0 + chunk));
      std::vector<uint32_t> dist, nh;
      const auto t0 = std::chrono::steady_clock::now();
      const std::vector<ospf_ctx*> cs = fromSweep ? std::vector<ospf_ctx*>{} : (ensureEngine(), slots());
      if (fromSweep) {
        sweepRows(part, W, dist, nh);
      } else if (cs.size() > 1 && part.size() >= cs.size()) {
        // split across the device slots: contiguous slices, rows in place
        const size_t m = part.size(), ns = cs.size();
        dist.assign(m * V, kInf);
        nh.assign(m * V * W, 0);
        const auto [rc, bad] = onSlots(cs, [&](size_t i, ospf_ctx* c) {
          const size_t a = m * i / ns, b = m * (i + 1) / ns;
          return b > a ? batchOn(c, part.data() + a, (uint32_t)(b - a), useLinkMetric,
                                 OSPF_WANT_DIST | OSPF_WANT_NH, W, dist.data() + a * V,
                                 nh.data() + a * V * W)
                       : OSPF_OK;
        });
        if (rc != OSPF_OK) throw EngineError(rc, ospf_last_error(cs[bad]));
        ++shardStats_.spf_batches;
        shardStats_.spf_launches += ns;
      } else {
        runBatch(part, nullptr, useLinkMetric, OSPF_WANT_DIST | OSPF_WANT_NH, W, &dist, &nh, nullptr);
      }
      const auto t1 = std::chrono::steady_clock::now();
      for (size_t i = 0; i < part.size(); ++i) {
        auto rows = std::make_shared<SpfRows>();
        rows->csr = csr_;
        rows->root = part[i];
        rows->W = W;
        rows->useLinkMetric = useLinkMetric;
        rows->dist.assign(dist.begin() + i * V, dist.begin() + (i + 1) * V);
        rows->nh.assign(nh.begin() + i * V * W, nh.begin() + (i + 1) * V * W);
        rows->nbrs = nbrsOf(part[i]);
        memo.emplace(csr_->names[part[i]], SpfResult(std::move(rows)));
      }
      if (knob_flag(Knob::ODL_SPF_TIMING)) {
        const auto t2 = std::chrono::steady_clock::now();
        fprintf(stderr, "spf_timing roots=%zu W=%u engine_ms=%.3f build_result_ms=%.3f\n",
                part.size(), W, std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(t2 - t1).count());
      }
    }
  }
}

std::vector<ospf_digest> LinkState::spfDigestsImpl(const std::vector<std::string>& roots,
                                                   bool useLinkMetric) {
  snapshot();
  std::vector<ospf_digest> out(roots.size(), ospf_digest{0, 0, 0});
  std::vector<uint32_t> ids;
  std::vector<size_t> pos;
  uint32_t W = 1;
  for (size_t i = 0; i < roots.size(); ++i) {
    ++spfRuns_;
    auto id = csr_->ids.find(roots[i]);
    if (id == csr_->ids.end()) {
      // root without a database: result {root: 0}; node_term(0xFFFFFFFF, 0)
      uint64_t x = (0xFFFFFFFFull << 32);
      x ^= x >> 30;
      x *= 0xbf58476d1ce4e5b9ULL;
      x ^= x >> 27;
      x *= 0x94d049bb133111ebULL;
      x ^= x >> 31;
      out[i] = ospf_digest{1, 0, x};
      continue;
    }
    if (hostRun(useLinkMetric)) {
      out[i] = digestHost(roots[i], runSpfHost(roots[i], useLinkMetric, {}));
      continue;
    }
    ids.push_back(id->second);
    pos.push_back(i);
    W = std::max(W, nhWordsFor(id->second));
  }
  if (!ids.empty()) {
    std::vector<ospf_digest> d;
    runBatch(ids, nullptr, useLinkMetric, OSPF_WANT_DIGEST, W, nullptr, nullptr, &d);
    for (size_t k = 0; k < ids.size(); ++k) out[pos[k]] = d[k];
  }
  return out;
}

std::optional<Metric> LinkState::getMetricFromAToB(const std::string& a, const std::string& b,
                                                   bool useLinkMetric) {
  if (a == b) return 0;
  const SpfResult& r = getSpfResult(a, useLinkMetric);
  auto it = r.find(b);
  if (it == r.end()) return std::nullopt;
  return it->second.metric();
}

std::shared_ptr<const SpfRows> LinkState::rawSpf(const std::string& node) {
  const SpfResult& r = getSpfResult(node, true);
  if (r.rows()) return r.rows();
  // a memoised result without engine rows: re-derive the distances (not a
  // new logical runSpf)
  snapshot();
  const uint32_t s = csr_->ids.at(node);
  auto rows = std::make_shared<SpfRows>();
  rows->csr = csr_;
  rows->root = s;
  runBatch({s}, nullptr, true, OSPF_WANT_DIST, nhWordsFor(s), &rows->dist, nullptr, nullptr);
  return rows;
}

std::optional<Path> LinkState::trace(const SpfRows& run, uint32_t src, uint32_t x,
                                     std::unordered_set<const Link*>& seen) const {
  if (x == src) return Path{};
  for (const auto& pl : run.pathLinksOf(x)) {
    if (!seen.insert(pl.link.get()).second) continue;
    auto p = trace(run, src, run.csr->ids.at(pl.prevNode), seen);
    if (p) {
      p->push_back(pl.link);
      return p;
    }
  }
  return std::nullopt;
}

std::vector<Path> LinkState::tracePaths(const SpfRows& run, uint32_t src, uint32_t dst) const {
  std::vector<Path> out;
  if (run.dist[dst] == kInf) return out;
  std::unordered_set<const Link*> seen;
  for (auto p = trace(run, src, dst, seen); p && !p->empty(); p = trace(run, src, dst, seen))
    out.push_back(std::move(*p));
  return out;
}

static std::string kspKey(const std::string& s, const std::string& d, size_t k) {
  std::string key = s;
  key += '\x01';
  key += d;
  key += '\x01';
  key += std::to_string(k);
  return key;
}

const std::vector<Path>& LinkState::getKthPathsImpl(const std::string& src, const std::string& dst,
                                                    size_t k) {
  if (k < 1) throw std::invalid_argument("k must be >= 1");
  const std::string key = kspKey(src, dst, k);
  auto it = memoKsp_.find(key);
  if (it != memoKsp_.end()) return it->second;
  std::unordered_set<const Link*> skipSet;
  std::vector<LinkPtr> skip;
  for (size_t i = 1; i < k; ++i)
    for (const auto& p : getKthPaths(src, dst, i))
      for (const auto& l : p)
        if (skipSet.insert(l.get()).second) skip.push_back(l);
  std::vector<Path> paths;
  snapshot();
  if (hostRun(true)) {
    if (skip.empty()) {
      paths = tracePathsHost(getSpfResult(src, true), src, dst);
    } else {
      ++spfRuns_;
      paths = tracePathsHost(runSpfHost(src, true, skipSet), src, dst);
    }
  } else if (skip.empty()) {
    const SpfResult& r = getSpfResult(src, true);
    if (r.count(dst) && csr_->ids.count(src)) {
      const auto run = rawSpf(src);
      paths = tracePaths(*run, run->csr->ids.at(src), run->csr->ids.at(dst));
    }
  } else {
    ++spfRuns_;
    snapshot();
    const uint32_t s = csr_->ids.at(src);
    std::vector<uint32_t> ign;
    for (const auto& l : skip) ign.push_back(linkIdOf(*l));
    std::sort(ign.begin(), ign.end());
    std::vector<uint32_t> dist;
    if (ign.size() <= OSPF_MAX_IGNORED_PER_RUN) {
      std::vector<std::vector<uint32_t>> igns{ign};
      runBatch({s}, &igns, true, OSPF_WANT_DIST, nhWordsFor(s), &dist, nullptr, nullptr);
    } else {
      // more ignored links than a run's list holds (e.g. the host side of a
      // KSP2 destination whose k = 1 paths overflowed the device record):
      // take them down on the device graph for this one run, then restore
      // (ospf_links_mask / unmask: the device graph and the engine's bounds
      // come back exactly as they were; on any failure the engine is marked
      // stale and reloaded by the next ensureEngine)
      ensureEngine();
      int rc = ospf_links_mask(engine_, ign.data(), (uint32_t)ign.size(), ~snapVersion_);
      if (rc != OSPF_OK) {
        const std::string m = ospf_last_error(engine_);
        ospf_links_unmask(engine_);
        engineVersion_ = 0;
        throw EngineError(rc, m);
      }
      dist.assign(V_of(*csr_), kInf);
      rc = ospf_sssp_batch(engine_, &s, 1, nullptr, OSPF_WANT_DIST, nhWordsFor(s), dist.data(),
                           nullptr, nullptr);
      const std::string m = rc != OSPF_OK ? ospf_last_error(engine_) : "";
      const int rc2 = ospf_links_unmask(engine_);
      if (rc != OSPF_OK || rc2 != OSPF_OK) {
        engineVersion_ = 0;
        throw EngineError(rc != OSPF_OK ? rc : rc2, rc != OSPF_OK ? m : ospf_last_error(engine_));
      }
    }
    SpfRows run;
    run.csr = csr_;
    run.root = s;
    run.dist = std::move(dist);
    run.ignored = std::move(ign);
    auto d = csr_->ids.find(dst);
    if (d != csr_->ids.end()) paths = tracePaths(run, s, d->second);
  }
  return memoKsp_.emplace(key, std::move(paths)).first->second;
}

void LinkState::prefetchKsp2Impl(const std::string& src, const std::vector<std::string>& dsts) {
  snapshot();
  if (hostRun(true)) {
    for (const auto& d : dsts) getKthPaths(src, d, 2);
    return;
  }
  auto sid = csr_->ids.find(src);
  std::vector<uint32_t> ids;
  std::vector<const std::string*> names;
  std::unordered_set<std::string> queued;
  for (const auto& d : dsts) {
    if (memoKsp_.count(kspKey(src, d, 2)) || !queued.insert(d).second) continue;
    auto did = csr_->ids.find(d);
    if (sid == csr_->ids.end() || did == csr_->ids.end()) {
      getKthPaths(src, d, 2);  // a side without an adjacency DB: no paths, host
      continue;
    }
    ids.push_back(did->second);
    names.push_back(&did->first);
  }
  if (ids.empty()) return;
  // k = 1 traces the memoised SPF of src (LinkState.cpp:804-805): one run
  getSpfResult(src, true);
  ensureEngine();
  // Device KSP2: SPF of src, k = 1 traces, masked reruns and k = 2 traces all
  // on the engine; records hold link ids. A destination over the engine's
  // budgets is computed by the host path below (same results, slower).
  uint32_t kCap = 1024;  // record words per destination and k
  kCap = (uint32_t)knob_int(Knob::ODL_KSP_CAP, (int)kCap);
  const size_t n = ids.size();
  std::vector<uint32_t> k1(n * kCap), k2(n * kCap), status(n);
  auto runOn = [&](ospf_ctx* c, size_t a0, size_t a1) {
    ospf_ksp2 a{};
    a.src = sid->second;
    a.dsts = ids.data() + a0;
    a.n = (uint32_t)(a1 - a0);
    a.path_cap = kCap;
    a.k1 = k1.data() + a0 * kCap;
    a.k2 = k2.data() + a0 * kCap;
    a.status = status.data() + a0;
    return a1 > a0 ? ospf_ksp2_run(c, &a) : OSPF_OK;
  };
  const std::vector<ospf_ctx*> cs = slots();
  if (cs.size() > 1 && n >= cs.size()) {
    // destinations of one source split across the device slots (SURVEY
    // §8(e)): each slot runs the source's SPF, its k = 1 traces and its
    // destinations' reruns; records land in place in k1 / k2 / status
    const size_t ns = cs.size();
    const auto [rc, bad] = onSlots(cs, [&](size_t i, ospf_ctx* c) {
      return runOn(c, n * i / ns, n * (i + 1) / ns);
    });
    if (rc != OSPF_OK) throw EngineError(rc, ospf_last_error(cs[bad]));
    ++shardStats_.ksp2_runs;
    shardStats_.ksp2_launches += ns;
  } else {
    const int rc = runOn(engine_, 0, n);
    if (rc != OSPF_OK) throw EngineError(rc, ospf_last_error(engine_));
  }
  auto decode = [&](const uint32_t* rec) {
    std::vector<Path> paths(rec[0]);
    for (uint32_t p = 0, q = 1; p < rec[0]; ++p) {
      const uint32_t len = rec[q];
      paths[p].reserve(len);
      for (uint32_t j = 0; j < len; ++j) paths[p].push_back(csr_->links.at(rec[q + 1 + j]));
      q += 1 + len;
    }
    return paths;
  };
  for (size_t i = 0; i < n; ++i) {
    const std::string& d = *names[i];
    if (!(status[i] & OSPF_KSP_OVF1)) memoKsp_.emplace(kspKey(src, d, 1), decode(&k1[i * kCap]));
    if (status[i] & (OSPF_KSP_OVF1 | OSPF_KSP_OVF2)) {
      getKthPaths(src, d, 2);
      continue;
    }
    if (status[i] & OSPF_KSP_RERUN) ++spfRuns_;  // runSpf(src, true, linksToIgnore)
    memoKsp_.emplace(kspKey(src, d, 2), decode(&k2[i * kCap]));
  }
}

// ---------------------------------------------------------------- incremental
void LinkState::applyIncremental(const std::vector<LinkDelta>& links,
                                 const std::vector<std::string>& nodes) {
  ++incStats_.patches;
  constexpr uint64_t kInf64 = ~0ull;
  auto distOf = [](const SpfResult& r, const std::string& n) -> uint64_t {
    auto it = r.find(n);
    return it == r.end() ? kInf64 : it->second.metric();
  };
  // the rule of ospf_affected_roots (include/openr_spf.h), on a memoised result
  auto affected = [&](const std::string& root, const SpfResult& r, bool hop) {
    for (const auto& d : links) {
      const Link& l = *d.link;
      const uint64_t da = distOf(r, l.lowNode()), db = distOf(r, l.highNode());
      const uint64_t w0ab = hop ? 1 : d.mlo0, w0ba = hop ? 1 : d.mhi0;
      const uint64_t w1ab = hop ? 1 : l.metricFrom(l.lowNode()),
                     w1ba = hop ? 1 : l.metricFrom(l.highNode());
      if (d.up0 && da != kInf64 && da + w0ab == db) return true;
      if (d.up0 && db != kInf64 && db + w0ba == da) return true;
      if (l.isUp() && da != kInf64 && da + w1ab <= db) return true;
      if (l.isUp() && db != kInf64 && db + w1ba <= da) return true;
    }
    for (const auto& x : nodes) {
      const uint64_t dx = distOf(r, x);
      if (dx == kInf64 || x == root) continue;
      for (const auto& l : linksFromNode(x)) {
        if (!l->isUp()) continue;
        if (dx + (hop ? 1 : l->metricFrom(x)) <= distOf(r, l->otherNode(x))) return true;
      }
    }
    return false;
  };
  // the dropped results go to the reaper thread, as clearMemo's do (a
  // route build's result holds ~100k materialised entries at F100k)
  auto dead = std::make_unique<MemoReaper::Dead>();
  for (int mode = 0; mode < 2; ++mode) {
    auto& memo = mode == 0 ? memoMetric_ : memoHops_;
    auto& to = mode == 0 ? dead->a : dead->b;
    for (auto it = memo.begin(); it != memo.end();) {
      if (affected(it->first, it->second, mode == 1)) {
        to.insert(memo.extract(it++));
        ++incStats_.dropped;
      } else {
        ++it;
        ++incStats_.kept;
      }
    }
  }
  dead->k.swap(memoKsp_);  // KSP2 masked reruns are not tracked
  if (!reaper_) {
    try {
      reaper_ = std::make_unique<MemoReaper>();
    } catch (const std::system_error&) {  // no thread to spare: freed here
    }
  }
  if (reaper_) reaper_->push(std::move(dead));
  patchGraph(links, nodes);
}

// The CSR and the device graph, patched in place (same node ids, same
// links): metrics, up state, overload bits.
void LinkState::patchGraph(const std::vector<LinkDelta>& links,
                           const std::vector<std::string>& nodes) {
  std::vector<ospf_link_update> ups;
  for (const auto& d : links) {
    const Link& l = *d.link;
    const uint32_t lid = linkIdOf(l);
    const uint32_t lo = csr_->ids.at(l.lowNode());
    auto clamp = [](Metric m) { return (m >= 1 && m <= 0xFFFFFFFFull) ? (uint32_t)m : 0u; };
    const uint32_t mlo = clamp(l.metricFrom(l.lowNode())), mhi = clamp(l.metricFrom(l.highNode()));
    for (uint32_t e = csr_->rowPtr[lo]; e < csr_->rowPtr[lo + 1]; ++e) {
      if (csr_->linkId[e] != lid) continue;
      const uint32_t t = csr_->twin[e];
      csr_->metric[e] = mlo;
      csr_->metric[t] = mhi;
      csr_->edgeUp[e] = csr_->edgeUp[t] = l.isUp() ? 1 : 0;
      break;
    }
    ups.push_back(ospf_link_update{lid, l.isUp() ? 1u : 0u, mlo, mhi});
    for (const std::string* n : {&l.lowNode(), &l.highNode()}) {  // largest in-range out-metric
      const uint32_t u = csr_->ids.at(*n);
      uint64_t mx = 0;
      for (const auto& x : linksFromNode(*n)) {
        const Metric m = x->metricFrom(*n);
        if (m >= 1 && m <= 0xFFFFFFFFull) mx = std::max<uint64_t>(mx, m);
      }
      csr_->rowMax[u] = mx;
    }
  }
  std::vector<uint32_t> nids;
  std::vector<uint8_t> nts;
  for (const auto& x : nodes) {
    const uint32_t id = csr_->ids.at(x);
    csr_->noTransit[id] = isNodeOverloaded(x) ? 1 : 0;
    nids.push_back(id);
    nts.push_back(csr_->noTransit[id]);
  }
  const bool inSync = engine_ && engineVersion_ == snapVersion_;
  ++version_;
  snapVersion_ = version_;
  dropSweep();  // its rows describe the graph before the patch
  if (inSync) {
    const uint32_t nctx = multi_ ? ospf_multi_size(multi_) : 1u;
    for (uint32_t i = 0; i < nctx; ++i) {
      ospf_ctx* c = multi_ ? ospf_multi_ctx(multi_, i) : engine_;
      int rc = ospf_update_links(c, ups.data(), (uint32_t)ups.size(), snapVersion_);
      if (rc == OSPF_OK) rc = ospf_update_nodes(c, nids.data(), nts.data(), (uint32_t)nids.size(),
                                                snapVersion_);
      if (rc != OSPF_OK) {
        engineVersion_ = 0;  // reload every device on the next use
        throw EngineError(rc, ospf_last_error(c));
      }
    }
    engineVersion_ = snapVersion_;
  }
}

// Links added / removed between known nodes, in place (LinkState.cpp:632-657
// [LINK UP] / [LINK DOWN]; node ids stay). The rows of the links' ends are
// rebuilt from their LinkSets (a set's iteration order -- the link ranks --
// may change on an insert), the arrays between them move as blocks, twins are
// remapped, and the engine patches the same rows (ospf_update_rows). O(E)
// block moves on host threads, no re-snapshot, no device reload.
void LinkState::patchStructure(const std::vector<LinkPtr>& added,
                               const std::vector<LinkPtr>& removed) {
  dropSweep();  // its rows describe the graph before the patch
  Csr& c = csrForWrite();
  const uint32_t V = (uint32_t)c.names.size();
  std::vector<uint32_t> rows;
  for (const auto* set : {&added, &removed})
    for (const auto& l : *set) {
      rows.push_back(c.ids.at(l->lowNode()));
      rows.push_back(c.ids.at(l->highNode()));
    }
  std::sort(rows.begin(), rows.end());
  rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
  for (const auto& l : removed) {
    const uint32_t lid = linkIdOf(*l);
    c.links[lid] = nullptr;
    c.freeLids.push_back(lid);
  }
  std::sort(c.freeLids.begin(), c.freeLids.end(), std::greater<uint32_t>());
  for (const auto& l : added) {
    uint32_t lid;
    if (!c.freeLids.empty()) {  // the smallest retired id
      lid = c.freeLids.back();
      c.freeLids.pop_back();
    } else {
      lid = (uint32_t)c.links.size();
      c.links.emplace_back();
    }
    c.links[lid] = l;
    l->snapLid = lid;
  }
  // the new rows, (neighbour id, rank) order
  struct Ent {
    uint32_t v, rank, metric, lid;
    uint8_t up;
  };
  const size_t K = rows.size();
  std::vector<std::vector<Ent>> nrow(K);
  for (size_t k = 0; k < K; ++k) {
    const uint32_t u = rows[k];
    const std::string& un = c.names[u];
    uint32_t rank = 0;
    uint64_t mx = 0;
    for (const auto& l : linksFromNode(un)) {
      const Metric m = l->metricOfEnd(l->endIndex(un));
      const bool inRange = m >= 1 && m <= 0xFFFFFFFFull;
      mx = std::max<uint64_t>(mx, inRange ? m : 0);
      nrow[k].push_back(Ent{c.ids.at(l->otherNode(un)), rank++, inRange ? (uint32_t)m : 1u,
                            l->snapLid, (uint8_t)(l->isUp() ? 1 : 0)});
    }
    std::sort(nrow[k].begin(), nrow[k].end(), [](const Ent& a, const Ent& b) {
      return a.v != b.v ? a.v < b.v : a.rank < b.rank;
    });
    c.rowMax[u] = mx;
  }
  // offsets: segment s (0..K) = the unchanged rows between changed rows
  // s - 1 and s, moved by shift[s]
  const std::vector<uint32_t> old = c.rowPtr;
  const size_t E0 = old[V];
  std::vector<int64_t> shift(K + 1, 0);
  for (size_t k = 0; k < K; ++k)
    shift[k + 1] = shift[k] + (int64_t)nrow[k].size() - (int64_t)(old[rows[k] + 1] - old[rows[k]]);
  const size_t E1 = (size_t)((int64_t)E0 + shift[K]);
  for (uint32_t u = 0, k = 0; u < V; ++u) {
    const bool ch = k < K && rows[k] == u;
    c.rowPtr[u + 1] = c.rowPtr[u] + (ch ? (uint32_t)nrow[k++].size() : old[u + 1] - old[u]);
  }
  auto segLo = [&](size_t s) { return s == 0 ? (size_t)0 : (size_t)old[rows[s - 1] + 1]; };
  auto segHi = [&](size_t s) { return s == K ? E0 : (size_t)old[rows[s]]; };
  auto move = [&](auto& a) {
    using T = typename std::decay_t<decltype(a)>::value_type;
    if (E1 > E0) a.resize(E1);
    for (size_t s = 1; s <= K; ++s)  // leftwards first, in order
      if (shift[s] < 0 && segHi(s) > segLo(s))
        std::memmove(a.data() + (int64_t)segLo(s) + shift[s], a.data() + segLo(s),
                     (segHi(s) - segLo(s)) * sizeof(T));
    for (size_t s = K; s >= 1; --s)  // then rightwards, from the end
      if (shift[s] > 0 && segHi(s) > segLo(s))
        std::memmove(a.data() + (int64_t)segLo(s) + shift[s], a.data() + segLo(s),
                     (segHi(s) - segLo(s)) * sizeof(T));
    if (E1 < E0) a.resize(E1);
  };
  std::vector<std::function<void()>> jobs = {[&] { move(c.col); }, [&] { move(c.metric); },
                                            [&] { move(c.linkId); }, [&] { move(c.twin); },
                                            [&] { move(c.linkRank); }, [&] { move(c.edgeUp); }};
  parallelFor((uint32_t)jobs.size(), [&](uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; ++j) jobs[j]();
  }, 1);
  // the rebuilt rows
  for (size_t k = 0; k < K; ++k) {
    size_t e = c.rowPtr[rows[k]];
    for (const Ent& x : nrow[k]) {
      c.col[e] = x.v;
      c.metric[e] = x.metric;
      c.linkId[e] = x.lid;
      c.linkRank[e] = x.rank;
      c.edgeUp[e] = x.up;
      c.twin[e] = kInf;
      ++e;
    }
  }
  // twins of unchanged entries: an old position in a segment moves with it;
  // one inside a changed row is set from that row below
  std::vector<uint32_t> starts(K);
  for (size_t k = 0; k < K; ++k) starts[k] = old[rows[k]];
  auto remap = [&](uint32_t t) -> uint32_t {
    const size_t i = (size_t)(std::upper_bound(starts.begin(), starts.end(), t) - starts.begin());
    if (i > 0 && t < old[rows[i - 1] + 1]) return kInf;  // inside changed row i - 1
    return (uint32_t)((int64_t)t + shift[i]);
  };
  for (size_t s = 0; s <= K; ++s) {
    const size_t lo = (size_t)((int64_t)segLo(s) + shift[s]), hi = (size_t)((int64_t)segHi(s) + shift[s]);
    if (hi <= lo) continue;
    parallelFor((uint32_t)(hi - lo), [&](uint32_t a, uint32_t b) {
      for (size_t e = lo + a; e < lo + b; ++e) c.twin[e] = remap(c.twin[e]);
    }, 1u << 16);
  }
  for (size_t k = 0; k < K; ++k) {
    const uint32_t u = rows[k];
    for (size_t e = c.rowPtr[u]; e < c.rowPtr[u + 1]; ++e) {
      if (c.twin[e] != kInf) continue;  // set from the partner row already
      const uint32_t x = c.col[e], lid = c.linkId[e];
      size_t q = c.rowPtr[x];
      while (q < c.rowPtr[x + 1] && !(c.linkId[q] == lid && q != e)) ++q;
      if (q == c.rowPtr[x + 1]) throw std::logic_error("patchStructure: link without a twin");
      c.twin[e] = (uint32_t)q;
      c.twin[q] = (uint32_t)e;
    }
  }
  uint64_t bound = 0;
  for (uint32_t u = 0; u < V; ++u) bound = std::min<uint64_t>(bound + c.rowMax[u], ~0ull >> 1);
  distBound_ = bound;
  ++topoStats_.link_patches;
  topoStats_.rows_patched += K;
  const bool inSync = engine_ && engineVersion_ == snapVersion_;
  ++version_;
  snapVersion_ = version_;
  if (inSync) patchEngineRows(rows);
}

LinkState::Csr& LinkState::csrForWrite() {
  // a kept memoised result reads this snapshot's ranks lazily: give it its own
  // (results handed to the reaper are no readers; only the live memo is)
  bool kept = false;
  for (const auto* m : {&memoMetric_, &memoHops_})
    for (const auto& kv : *m) kept |= kv.second.rows() && kv.second.rows()->csr == csr_;
  if (kept) csr_ = std::make_shared<Csr>(*csr_);
  return *csr_;
}

void LinkState::csrInsertNode(uint32_t k, const std::string& name, bool overloaded) {
  Csr& c = csrForWrite();
  const uint32_t V = (uint32_t)c.names.size();
  if (k > V) throw std::logic_error("csrInsertNode: position");
  c.names.insert(c.names.begin() + k, name);
  for (auto& kv : c.ids)
    if (kv.second >= k) ++kv.second;
  c.ids.emplace(name, k);
  c.rowPtr.insert(c.rowPtr.begin() + k + 1, c.rowPtr[k]);  // an empty row k
  parallelFor((uint32_t)c.col.size(), [&](uint32_t lo, uint32_t hi) {
    for (uint32_t e = lo; e < hi; ++e)
      if (c.col[e] >= k && c.col[e] != kInf) ++c.col[e];
  }, 1u << 16);
  c.noTransit.insert(c.noTransit.begin() + k, overloaded ? 1 : 0);
  c.rowMax.insert(c.rowMax.begin() + k, 0);
  ++topoStats_.node_patches;
}

void LinkState::csrEraseNode(uint32_t k) {
  Csr& c = csrForWrite();
  if (k >= c.names.size() || c.rowPtr[k] != c.rowPtr[k + 1])
    throw std::logic_error("csrEraseNode: row not empty");
  c.ids.erase(c.names[k]);
  for (auto& kv : c.ids)
    if (kv.second > k) --kv.second;
  c.names.erase(c.names.begin() + k);
  c.rowPtr.erase(c.rowPtr.begin() + k + 1);
  parallelFor((uint32_t)c.col.size(), [&](uint32_t lo, uint32_t hi) {
    for (uint32_t e = lo; e < hi; ++e)
      if (c.col[e] > k && c.col[e] != kInf) --c.col[e];
  }, 1u << 16);
  c.noTransit.erase(c.noTransit.begin() + k);
  c.rowMax.erase(c.rowMax.begin() + k);
  ++topoStats_.node_patches;
}

void LinkState::patchEngineRows(const std::vector<uint32_t>& rows) {
  const Csr& c = *csr_;
  ospf_csr g{};
  g.n_nodes = (uint32_t)c.names.size();
  g.n_edges = (uint32_t)c.col.size();
  g.row_ptr = c.rowPtr.data();
  g.col = c.col.data();
  g.metric = c.metric.data();
  g.link_id = c.linkId.data();
  g.twin = c.twin.data();
  g.edge_up = c.edgeUp.data();
  g.no_transit = c.noTransit.data();
  g.link_rank = c.linkRank.data();
  const uint32_t nctx = multi_ ? ospf_multi_size(multi_) : 1u;
  for (uint32_t i = 0; i < nctx; ++i) {
    ospf_ctx* x = multi_ ? ospf_multi_ctx(multi_, i) : engine_;
    const int rc = ospf_update_rows(x, &g, rows.data(), (uint32_t)rows.size(), snapVersion_);
    if (rc == OSPF_E_RANGE) {  // the device layout's reserve is spent: reload
      engineVersion_ = 0;
      return;
    }
    if (rc != OSPF_OK) {
      engineVersion_ = 0;  // reload every device on the next use
      throw EngineError(rc, ospf_last_error(x));
    }
  }
  engineVersion_ = snapVersion_;
}

void NodeUcmpResult::normalizeNextHopWeights() {
  int64_t g = 0;
  for (const auto& kv : nextHopLinks_) g = std::gcd(g, kv.second.weight);
  if (g > 1)
    for (auto& kv : nextHopLinks_) kv.second.weight /= g;
}

UcmpResult LinkState::resolveUcmpWeights(
    const SpfResult& spfGraph, const std::unordered_map<std::string, int64_t>& leafNodeToWeights,
    UcmpAlgo algo, bool useLinkMetric) const {
  // decision.ucmp_runs / ucmp_ms (LinkState.cpp:926,1025-1029)
  struct Timer {
    Counters& c;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~Timer() {
      ++c.ucmp_runs;
      c.ucmp_ms_sum +=
          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  } timer{counters_};
  UcmpResult out;
  // DijkstraQ<DijkstraQUcmpNode> (LinkState.h:573-645): entries still queued,
  // by name; pop order (metric, name). A popped node leaves the map, so a later
  // path link to it queues it again, as in the reference.
  struct Item {
    Metric metric;
    NodeUcmpResult result;
  };
  std::unordered_map<std::string, Item> queued;
  std::set<std::pair<Metric, std::string>> order;
  auto insert = [&](const std::string& n, Metric m) {
    queued[n] = Item{m, NodeUcmpResult{}};
    order.emplace(m, n);
  };
  // leaves present in the SPF graph, all at the same distance from the root
  // (LinkState.cpp:937-959)
  std::optional<Metric> spfMetric;
  for (const auto& [leaf, weight] : leafNodeToWeights) {
    auto it = spfGraph.find(leaf);
    if (it == spfGraph.end()) continue;
    const Metric m = it->second.metric();
    if (!spfMetric) {
      spfMetric = m;
    } else if (*spfMetric != m) {
      return UcmpResult{};  // "Skipping resolveUcmpWeights"
    }
    insert(leaf, 0);
    queued.at(leaf).result.setWeight(weight);
  }
  // walk from the leaves towards the root (LinkState.cpp:961-1023)
  while (!order.empty()) {
    const auto [metric, name] = *order.begin();
    order.erase(order.begin());
    NodeUcmpResult cur = std::move(queued.at(name).result);
    queued.erase(name);
    if (!cur.weight()) {
      int64_t advertised = 0;
      for (const auto& [iface, nh] : cur.nextHopLinks())
        advertised += algo == UcmpAlgo::kAdjWeightPropagation ? nh.link->weightFrom(name)
                                                              : nh.weight;
      cur.setWeight(advertised);
    }
    auto sit = spfGraph.find(name);
    if (sit == spfGraph.end()) throw std::logic_error("UCMP node not in the SPF graph");
    for (const auto& pl : sit->second.pathLinks()) {
      const Metric lm = useLinkMetric ? pl.link->metricFrom(pl.prevNode) : 1;
      auto q = queued.find(pl.prevNode);
      if (q == queued.end()) {
        insert(pl.prevNode, metric + lm);
        q = queued.find(pl.prevNode);
      }
      q->second.result.addNextHopLink(pl.link->ifaceFrom(pl.prevNode), pl.link, name,
                                      *cur.weight());
    }
    cur.normalizeNextHopWeights();
    out.emplace(name, std::move(cur));
  }
  return out;
}

// ---------------------------------------------------------------- host path
SpfResult LinkState::runSpfHost(const std::string& root, bool useLinkMetric,
                                const std::unordered_set<const Link*>& ignore) const {
  // Dijkstra with the reference's queue order -- (metric, name), keys only
  // ever lowered by a strictly better path -- and its u64 arithmetic, so a
  // wrapped negative metric behaves exactly as there.
  SpfResult::Map done;
  std::unordered_map<std::string, NodeSpfResult> open;
  std::set<std::pair<Metric, std::string>> order;
  open.emplace(root, NodeSpfResult(0));
  order.emplace(0, root);
  while (!order.empty()) {
    const std::string name = order.begin()->second;
    order.erase(order.begin());
    auto node = open.find(name);
    auto& rec = done.emplace(name, std::move(node->second)).first->second;
    open.erase(node);
    if (name != root && isNodeOverloaded(name)) continue;  // no transit
    for (const auto& link : linksFromNode(name)) {
      const std::string& other = link->otherNode(name);
      if (!link->isUp() || done.count(other) || ignore.count(link.get())) continue;
      const Metric cand = rec.metric() + (useLinkMetric ? link->metricFrom(name) : 1);
      auto it = open.find(other);
      if (it == open.end()) {
        it = open.emplace(other, NodeSpfResult(cand)).first;
        order.emplace(cand, other);
      }
      NodeSpfResult& o = it->second;
      if (o.metric() < cand) continue;
      if (o.metric() > cand) {  // strictly better: forget the other paths
        order.erase({o.metric(), other});
        o = NodeSpfResult(cand);
        order.emplace(cand, other);
      }
      o.pathLinks_.push_back(PathLink{link, name});
      o.nextHops_.insert(rec.nextHops_.begin(), rec.nextHops_.end());
      if (o.nextHops_.empty()) o.nextHops_.insert(other);  // a neighbour of the root
    }
  }
  return SpfResult(std::move(done));
}

std::vector<Path> LinkState::tracePathsHost(const SpfResult& res, const std::string& src,
                                            const std::string& dst) const {
  std::vector<Path> out;
  if (!res.count(dst)) return out;
  std::unordered_set<const Link*> seen;
  std::function<std::optional<Path>(const std::string&)> one =
      [&](const std::string& x) -> std::optional<Path> {
    if (x == src) return Path{};
    for (const auto& pl : res.at(x).pathLinks()) {
      if (!seen.insert(pl.link.get()).second) continue;
      auto p = one(pl.prevNode);
      if (p) {
        p->push_back(pl.link);
        return p;
      }
    }
    return std::nullopt;
  };
  for (auto p = one(dst); p && !p->empty(); p = one(dst)) out.push_back(std::move(*p));
  return out;
}

ospf_digest LinkState::digestHost(const std::string& root, const SpfResult& res) const {
  // the engine's digest with u64 distances: node ids and the
  // root's neighbour bit positions of the current snapshot
  auto mix = [](uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
  };
  const uint32_t r = csr_->ids.at(root);
  std::unordered_map<std::string, uint32_t> bit;
  for (uint32_t e = csr_->rowPtr[r]; e < csr_->rowPtr[r + 1]; ++e) {
    const uint32_t v = csr_->col[e];
    if (v != r && !bit.count(csr_->names[v])) {
      const uint32_t i = (uint32_t)bit.size();
      bit.emplace(csr_->names[v], i);
    }
  }
  ospf_digest d{0, 0, 0};
  for (const auto& [name, nr] : res) {
    const uint32_t v = csr_->ids.at(name);
    const uint64_t kd = mix((uint64_t)v ^ 0x2545F4914F6CDD1DULL) | 1ull;
    const uint64_t kn = mix((uint64_t)v ^ 0xD6E8FEB86659FD93ULL) | 1ull;
    std::map<uint32_t, uint32_t> words;
    for (const auto& h : nr.nextHops()) {
      const uint32_t i = bit.at(h);
      words[i / 32] |= 1u << (i % 32);
    }
    uint64_t ws = 0;
    for (const auto& [w, word] : words)
      if (word) ws += mix((((uint64_t)w << 32) | word) ^ 0x9E3779B97F4A7C15ULL);
    d.reached += 1;
    d.sum_dist += nr.metric();
    d.hash += kd * (nr.metric() + 1) + kn * ws;
  }
  return d;
}

bool LinkState::pathAInPathB(const Path& a, const Path& b) {
  if (a.size() > b.size()) return false;
  for (size_t i = 0; i + a.size() <= b.size(); ++i) {
    size_t k = 0;
    while (k < a.size() && a[k]->sameLink(*b[i + k])) ++k;
    if (k == a.size()) return true;
  }
  return false;
}

}  // namespace odl
