// unipeak_amd/host/engine.cpp -- see engine.hpp.
#include "engine.hpp"
#include "cli.hpp"
#include "bbi.hpp"

#include <algorithm>
#include <unordered_map>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <thread>

namespace unipeak {

// countSum of one add (peakcall.cpp:186-200, quirk Q5): only used here to
// spot head hits; the device recomputes it bit-exactly from the tracks
static double count_sum(const uint32_t *c, size_t S, const std::vector<uint8_t> &control,
                        const std::vector<double> &coeffs) {
    double s = 0;
    if (coeffs.empty()) {
        for (size_t i = 0; i < S; ++i)
            if (!control[i]) s += (double)c[i];
    } else {
        size_t k = 0;
        for (size_t i = 0; i < S && k < coeffs.size(); ++i)
            if (!control[i]) s += (double)c[i] * coeffs[k++];
        for (size_t i = 0; i < S; ++i)
            if (!control[i]) s += (double)c[i];
    }
    return s;
}

namespace {

// one driver-loop iteration (a contig pass): the units it creates and the
// number of add() calls, with add times on a clock local to the iteration
struct IterOut {
    std::vector<UnitBuild> units;
    uint64_t adds = 0;
    bool stepped = false;  // the position loop ran at least once
};

struct MergeSpec {
    size_t S;
    bool directional;
    uint16_t bw;
    const std::vector<uint8_t> *control;
    const std::vector<double> *coeffs;
};

// the position loop of one iteration, src/regions.cpp:311-371 (and
// src/strand_shift.cpp:144-186): every stream whose head lies on this contig
// is consumed position by position; head(i) is stream i's current record,
// advance(i) reads its next one
template <class Head, class Advance>
void merge_iteration(const MergeSpec &m, uint32_t contig, uint32_t lim, uint32_t iteration,
                     uint32_t len, Head head, Advance advance, IterOut &o, uint64_t reserve = 0) {
    const size_t S = m.S;
    std::vector<uint32_t> fh(S), rh(S);
    int cur[2] = {-1, -1};
    auto add = [&](int buffer, int strand, const std::vector<uint32_t> &counts, uint32_t pos) {
        if (cur[buffer] < 0) {
            UnitBuild u;
            u.buffer = buffer;
            u.contig = contig;
            u.len = len;
            u.iteration = iteration;
            if (reserve) {
                const int tr = m.directional ? 0 : strand;
                u.pos[tr].reserve(reserve);
                u.cnt[tr].reserve(reserve * S);
                u.add_pos.reserve(reserve);
                u.add_time.reserve(reserve);
            }
            o.units.push_back(std::move(u));
            cur[buffer] = (int)o.units.size() - 1;
        }
        UnitBuild &u = o.units[cur[buffer]];
        const int track = m.directional ? 0 : strand;
        u.pos[track].push_back(pos);
        for (size_t i = 0; i < S; ++i) u.cnt[track].push_back(counts[i]);
        u.add_pos.push_back(pos);
        u.add_time.push_back(++o.adds);
        if (pos <= m.bw && count_sum(counts.data(), S, *m.control, *m.coeffs) != 0) u.head_hit = true;
    };
    uint32_t pos = 1;
    while (pos <= lim) {
        o.stepped = true;
        bool ff = false, fr = false;
        uint32_t next = lim + 1;
        for (size_t i = 0; i < S; ++i) {
            fh[i] = 0;
            rh[i] = 0;
            const auto *a = &head(i);
            while (a->count != 0 && a->first == pos && a->contig == contig) {
                if (a->forward) { fh[i] += a->count; ff = true; }
                else { rh[i] += a->count; fr = true; }
                a = &advance(i);
            }
            if (a->count != 0 && a->contig == contig && a->first < next) next = a->first;
        }
        if (ff) add(0, 0, fh, pos);
        if (fr) add(m.directional ? 1 : 0, 1, rh, pos);
        pos = next;
    }
    // flushContig(): forward buffer (local time adds+1), then reverse (adds+2)
    for (int b = 0; b < 2; ++b)
        if (cur[b] >= 0) o.units[cur[b]].flush_time = o.adds + 1 + b;
}

// the driver's iteration sequence: contig of iteration i
struct Iterations {
    uint32_t nc;
    bool directional;
    uint32_t count() const { return directional ? 2 * nc : nc; }
    uint32_t contig(uint32_t i) const { return i % nc; }
};

// concatenate iterations on the global event clock: each add ticks once,
// each iteration ends with two flush ticks
void stitch(std::vector<IterOut> &its, PassResult &out) {
    uint64_t base = 0;
    for (IterOut &o : its) {
        for (UnitBuild &u : o.units) {
            for (uint64_t &t : u.add_time) t += base;
            if (u.flush_time) u.flush_time += base;
            out.units.push_back(std::move(u));
        }
        if (o.stepped) out.last_write = base + o.adds;
        base += o.adds + 2;
    }
}

// a stream decoded ahead of the merge: every record read_align() returns
// (the record already read by the caller first), then the count-0 end
using Rec = Tag;

struct Decoded {
    std::unique_ptr<SampleStream> stream;
    std::vector<Rec> recs;
    bool ok = false;
};

void decode_stream(const SampleStream &orig, Decoded &d, unsigned threads) {
    t_defer_errors = true;
    try {
        d.stream = orig.reopen();
        d.stream->expected_tags();
        d.recs.reserve(d.stream->size_hint() + 1);
        const Align *a = &d.stream->read_align();  // the caller's first read
        if (a->count != 0) {
            d.recs.push_back(Rec{a->contig, a->first, a->count, a->forward});
            if (!d.stream->decode_rest(d.recs, threads)) {  // nondirectional: record by record
                for (a = &d.stream->read_align(); a->count != 0; a = &d.stream->read_align())
                    d.recs.push_back(Rec{a->contig, a->first, a->count, a->forward});
            }
        }
        d.recs.push_back(Rec{0, 0, 0, true});
        d.ok = true;
    } catch (const DeferredError &) {
        d.ok = false;
    }
    t_defer_errors = false;
}

}  // namespace

void build_units(std::vector<SampleStream *> &streams, const ContigTable &ct, bool directional,
                 uint16_t bw, const std::vector<uint8_t> &control, const std::vector<double> &coeffs,
                 bool quiet, PassResult &out) {
    (void)quiet;
    const size_t S = streams.size();
    const MergeSpec m{S, directional, bw, &control, &coeffs};
    const Iterations itn{ct.size(), directional};
    const unsigned T = ingest_threads();

    // (1) decode every stream ahead, one thread per stream
    std::vector<Decoded> dec(S);
    const char *ser = std::getenv("UNIPEAK_SERIAL_INGEST");
    bool parallel = !(ser && *ser && *ser != '0');
    if (parallel) {
        std::vector<std::thread> pool;
        std::atomic<size_t> next{0};
        const unsigned outer = (unsigned)std::min<size_t>(T, S), inner = std::max(1u, T / outer);
        for (unsigned t = 0; t < outer; ++t)
            pool.emplace_back([&] {
                for (size_t i; (i = next.fetch_add(1)) < S;) decode_stream(*streams[i], dec[i], inner);
            });
        for (auto &th : pool) th.join();
    }
    // (2) which iteration consumes each run of same-contig records: the
    // first one after the previous run's whose contig matches.  A run no
    // iteration reaches leaves its stream stuck there; that case, and any
    // input error, goes to the serial replay below.
    std::vector<std::vector<std::pair<size_t, size_t>>> slice(
        itn.count(), std::vector<std::pair<size_t, size_t>>(S, {0, 0}));
    for (size_t i = 0; i < S && parallel; ++i) {
        const Decoded &d = dec[i];
        if (!d.ok) { parallel = false; break; }
        const size_t n = d.recs.size() - 1;
        int64_t prev = -1;
        for (size_t b = 0; b < n;) {
            const uint32_t c = d.recs[b].contig;
            size_t e = b + 1;
            while (e < n && d.recs[e].contig == c) ++e;
            int64_t it = -1;
            for (uint32_t k = (uint32_t)(prev + 1); k < itn.count(); ++k)
                if (itn.contig(k) == c) { it = k; break; }
            if (it < 0) { parallel = false; break; }
            slice[it][i] = {b, e};
            prev = it;
            b = e;
        }
    }
    std::vector<IterOut> its(itn.count());
    if (parallel) {
        // (3) iterations in parallel, each over its slices of the records
        std::vector<uint32_t> order(itn.count());
        for (uint32_t k = 0; k < itn.count(); ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return ct.length(itn.contig(a)) > ct.length(itn.contig(b));
        });
        std::vector<std::thread> pool;
        std::atomic<size_t> next{0};
        for (unsigned t = 0; t < std::min<size_t>(T, order.size()); ++t)
            pool.emplace_back([&] {
                std::vector<size_t> at(S);
                for (size_t j; (j = next.fetch_add(1)) < order.size();) {
                    const uint32_t k = order[j];
                    for (size_t i = 0; i < S; ++i) at[i] = slice[k][i].first;
                    auto head = [&](size_t i) -> const Rec & {
                        const Decoded &d = dec[i];
                        return at[i] < slice[k][i].second ? d.recs[at[i]] : d.recs.back();
                    };
                    auto advance = [&](size_t i) -> const Rec & {
                        ++at[i];
                        return head(i);
                    };
                    const uint32_t c = itn.contig(k);
                    uint64_t bound = 0;  // adds per buffer are at most the records consumed
                    for (size_t i = 0; i < S; ++i) bound += slice[k][i].second - slice[k][i].first;
                    merge_iteration(m, c, ct.length(c), k, ct.length(c), head, advance, its[k], bound);
                }
            });
        for (auto &th : pool) th.join();
        // the callers' streams continue from where the decode left them (EOF)
        for (size_t i = 0; i < S; ++i) *streams[i] = std::move(*dec[i].stream);
    } else {
        // serial replay on the callers' streams, exactly as the reference reads
        for (uint32_t k = 0; k < itn.count(); ++k) {
            const uint32_t c = itn.contig(k);
            merge_iteration(
                m, c, ct.length(c), k, ct.length(c),
                [&](size_t i) -> const Align & { return streams[i]->last(); },
                [&](size_t i) -> const Align & { return streams[i]->read_align(); }, its[k]);
        }
    }
    dec.clear();
    stitch(its, out);
    out.parallel_ingest = parallel;
}

template <class V>
static uint64_t fnv(const V &v) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char *p = (const unsigned char *)v.data();
    for (size_t i = 0; i < v.size() * sizeof(v[0]); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

void maybe_dump_units(const PassResult &pr, const std::vector<SampleStream *> &streams) {
    const char *path = std::getenv("UNIPEAK_DUMP_UNITS");
    if (!path || !*path) return;
    FILE *f = std::fopen(path, "w");
    if (!f) fatal(std::string("could not write ") + path);
    std::fprintf(f, "ingest %s\n", pr.parallel_ingest ? "parallel" : "serial");
    std::fprintf(f, "last_write %llu\n", (unsigned long long)pr.last_write);
    for (const UnitBuild &u : pr.units)
        std::fprintf(f, "unit b%d c%u it%u len%u flush%llu head%d n%zu/%zu %016llx %016llx %016llx %016llx %016llx %016llx\n",
                     u.buffer, u.contig, u.iteration, u.len, (unsigned long long)u.flush_time,
                     (int)u.head_hit, u.pos[0].size(), u.pos[1].size(),
                     (unsigned long long)fnv(u.pos[0]), (unsigned long long)fnv(u.pos[1]),
                     (unsigned long long)fnv(u.cnt[0]), (unsigned long long)fnv(u.cnt[1]),
                     (unsigned long long)fnv(u.add_pos), (unsigned long long)fnv(u.add_time));
    for (SampleStream *s : streams)
        std::fprintf(f, "stream %s expected %llu confident %llu oob %llu\n", s->expt_name().c_str(),
                     (unsigned long long)s->expected_tags(), (unsigned long long)s->confident(),
                     (unsigned long long)s->out_of_bounds());
    std::fclose(f);
    exit_now(0);
}

namespace {

struct DeviceJob {
    int dev;
    std::vector<uint32_t> units;  // global unit indices
    up_ctx *ctx = nullptr;
    std::vector<uint32_t> dev_unit;  // device unit id -> global unit index
    std::vector<uint64_t> cand_idx;  // candidate list index of each device region
    int rc = UP_OK;
    std::string err;
};

std::vector<DeviceJob> g_jobs;  // kept alive for shift_scan

void check(int rc, const char *what) {
    if (rc != UP_OK) fatal(std::string(what) + ": " + up_strerror(rc));
}

}  // namespace

// device contexts opened ahead, while the host parses (HIP runtime start-up
// and context creation overlap ingest); run_units takes them over
namespace {
std::thread g_prewarm;
std::vector<up_ctx *> g_pre;
int g_pre_ndev = 0;
}  // namespace

static void join_prewarm() {
    if (g_prewarm.joinable()) g_prewarm.join();
}

void prewarm_devices(int ngpus) {
    g_exit_hook = join_prewarm;  // an input error must not exit mid-initialisation
    (void)ngpus;  // cli_device_count() reads UNIPEAK_GPUS / UNIPEAK_SHARE_DEVICE
    g_prewarm = std::thread([] {
        const int nd = cli_device_count();
        std::vector<up_ctx *> pre(std::max(nd, 0), nullptr);
        for (int d = 0; d < nd; ++d)
            if (up_open(cli_physical_device(d), &pre[d]) != UP_OK) pre[d] = nullptr;
        g_pre = std::move(pre);
        g_pre_ndev = nd;
    });
}

void run_units(const EngineParams &ep, PassResult &out) {
    int ndev = 0;
    if (g_prewarm.joinable()) {
        g_prewarm.join();
        ndev = g_pre_ndev;
    } else {
        ndev = cli_device_count();
    }
    if (ndev < 1) fatal("no HIP device available (the GPU path has no CPU fallback)");
    const size_t S = ep.p.n_samples;
    // Quirk Q1: a unit whose adds all sit at positions <= bw leaves density
    // (and maybe an open region) in its buffer after flushContig(); the
    // library replays such chains, so a chain's units share one device.
    // With a region threshold <= 0 (quirk Q11 live) every unit's last region
    // is still open after its flush and is closed -- relabelled -- in the
    // buffer's next unit (peakcall.cpp:76-78, 164-168), so every unit of a
    // buffer chains to the next one.
    // group[i] = first unit of the chain unit i belongs to.
    std::vector<uint32_t> group(out.units.size());
    {
        const bool q11 = !(ep.p.region_thr > 0);
        int32_t open_prev[2] = {-1, -1};
        for (uint32_t i = 0; i < out.units.size(); ++i) {
            const UnitBuild &u = out.units[i];
            const int b = u.buffer;
            const bool linked = open_prev[b] >= 0;
            group[i] = linked ? group[open_prev[b]] : i;
            const bool in_chain = u.head_hit || linked;
            const bool leaks = !u.add_pos.empty() && u.add_pos.back() <= ep.p.bw;
            open_prev[b] = (q11 || (in_chain && leaks)) ? (int32_t)i : -1;
        }
    }
    // LPT assignment of unit groups to devices by track bytes
    const int nstr = ep.p.nondir ? 2 : 1;
    std::vector<uint64_t> gbytes(out.units.size(), 0);
    for (uint32_t i = 0; i < out.units.size(); ++i)
        gbytes[group[i]] += (uint64_t)out.units[i].len * nstr * S;
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < out.units.size(); ++i)
        if (group[i] == i) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return gbytes[a] > gbytes[b]; });
    std::vector<uint64_t> load(ndev, 0);
    std::vector<int> gdev(out.units.size(), 0);
    g_jobs.assign(ndev, DeviceJob());
    for (int d = 0; d < ndev; ++d) g_jobs[d].dev = d;
    for (uint32_t g : order) {
        int best = 0;
        for (int d = 1; d < ndev; ++d)
            if (load[d] < load[best]) best = d;
        load[best] += gbytes[g];
        gdev[g] = best;
    }
    for (uint32_t i = 0; i < out.units.size(); ++i) g_jobs[gdev[group[i]]].units.push_back(i);
    for (auto &j : g_jobs) std::sort(j.units.begin(), j.units.end());  // buffer order kept

    std::mutex mu;
    auto work = [&](DeviceJob &job) {
        auto fail = [&](int rc, const char *what) {
            job.rc = rc;
            job.err = std::string(what) + ": " + up_strerror(rc);
        };
        if (job.units.empty()) return;
        PhaseTimer tm;
        int rc = UP_OK;
        if (job.dev < (int)g_pre.size() && g_pre[job.dev]) {
            job.ctx = g_pre[job.dev];
            g_pre[job.dev] = nullptr;
        } else if ((rc = up_open(cli_physical_device(job.dev), &job.ctx))) {
            return fail(rc, "up_open");
        }
        tm.mark("  gpu: up_open");
        up_params p = ep.p;
        p.is_control = ep.control.data();
        p.coeffs = ep.coeffs.empty() ? nullptr : ep.coeffs.data();
        p.n_coeffs = (uint32_t)ep.coeffs.size();
        if ((rc = up_set_params(job.ctx, &p))) return fail(rc, "up_set_params");
        if (ep.profile && (rc = up_set_profile_capture(job.ctx, 1))) return fail(rc, "up_set_profile_capture");
        // (-D above bw 511: K1w and the profile kernel with the capture on, not the whole-buffer replay)
        if ((rc = up_set_wide_nd_full(job.ctx, 1))) return fail(rc, "up_set_wide_nd_full");
        // (-D above bw 511 at -r <= 0: wide K1q, not the segmented replay)
        if ((rc = up_set_wide_q11_nd(job.ctx, 1))) return fail(rc, "up_set_wide_q11_nd");
        // (head units of a -s run: replayed and merged on the device, inside the pass)
        if ((rc = up_set_head_place(job.ctx, 1))) return fail(rc, "up_set_head_place");
        std::vector<uint32_t> tp, tc;
        for (uint32_t gi : job.units) {
            const UnitBuild &u = out.units[gi];
            uint32_t id = 0;
            if ((rc = up_add_unit(job.ctx, u.len, nstr, u.buffer, &id))) return fail(rc, "up_add_unit");
            tm.accumulate(0);
            job.dev_unit.push_back(gi);
            for (int st = 0; st < nstr; ++st) {
                const size_t n = u.pos[st].size();
                if (S == 1) {  // every add of a single sample carries a nonzero count
                    if (n && (rc = up_unit_scatter(job.ctx, id, st, 0, n, u.pos[st].data(), u.cnt[st].data())))
                        return fail(rc, "up_unit_scatter");
                    continue;
                }
                for (size_t s = 0; s < S; ++s) {
                    tp.clear();
                    tc.clear();
                    for (size_t k = 0; k < n; ++k) {
                        const uint32_t c = u.cnt[st][k * S + s];
                        if (c) {
                            tp.push_back(u.pos[st][k]);
                            tc.push_back(c);
                        }
                    }
                    if (!tp.empty() &&
                        (rc = up_unit_scatter(job.ctx, id, st, (uint16_t)s, tp.size(), tp.data(), tc.data())))
                        return fail(rc, "up_unit_scatter");
                }
            }
            if (!u.add_pos.empty()) up_unit_set_last_add(job.ctx, id, u.add_pos.back());
            tm.accumulate(1);
        }
        tm.report(0, "  gpu: up_add_unit");
        tm.report(1, "  gpu: scatter");
        tm.mark("  gpu: units + scatter");
        uint64_t n = 0;
        if ((rc = up_run(job.ctx, &n))) return fail(rc, "up_run");
        tm.mark("  gpu: up_run");
        std::vector<up_region> regs(n);
        std::vector<uint32_t> cnt(n * S);
        if (n && (rc = up_get_regions(job.ctx, regs.data(), cnt.data(), n))) return fail(rc, "up_get_regions");
        tm.mark("  gpu: fetch");
        std::lock_guard<std::mutex> lk(mu);
        for (uint64_t i = 0; i < n; ++i) {
            Candidate c;
            c.r = regs[i];
            c.unit_index = job.dev_unit[regs[i].unit];
            c.counts.assign(cnt.begin() + i * S, cnt.begin() + (i + 1) * S);
            job.cand_idx.push_back(out.cands.size());
            out.cands.push_back(std::move(c));
        }
    };
    std::vector<std::thread> th;
    for (auto &j : g_jobs) th.emplace_back(work, std::ref(j));
    for (auto &t : th) t.join();
    for (auto &j : g_jobs)
        if (j.rc != UP_OK) fatal("GPU device " + std::to_string(j.dev) + ": " + j.err);
}

std::vector<Emitted> order_candidates(const PassResult &out, uint16_t bw, bool accepted_only) {
    std::vector<Emitted> v;
    v.reserve(out.cands.size());
    const uint64_t last_write = out.last_write;
    for (const Candidate &c : out.cands) {
        const UnitBuild &u = out.units[c.unit_index];
        // closed by the first add at pos >= right + bw + 2, else by the flush;
        // regions from the Q1 replay name their closing add (0: the flush);
        // threshold <= 0 (Q11): by the first add past the first add at pos >=
        // right + bw + 1, or (a region left open by the previous unit) past
        // the unit's first add -- an add at the same position (the other
        // strand) retires nothing
        uint64_t key = (uint64_t)c.r.right + bw + 2;
        if (c.r.close_pos == UP_CLOSE_Q11 || c.r.close_pos == UP_CLOSE_Q11_HEAD) {
            auto a1 = u.add_pos.begin();
            if (c.r.close_pos == UP_CLOSE_Q11)
                a1 = std::lower_bound(u.add_pos.begin(), u.add_pos.end(), (uint64_t)c.r.right + bw + 1,
                                      [](uint32_t a, uint64_t k) { return (uint64_t)a < k; });
            key = a1 != u.add_pos.end() ? (uint64_t)*a1 + 1 : ~0ull;
        } else if (c.r.close_pos != UP_CLOSE_RULE) {
            key = c.r.close_pos ? c.r.close_pos : ~0ull;
        }
        auto it = std::lower_bound(u.add_pos.begin(), u.add_pos.end(), key,
                                   [](uint32_t a, uint64_t k) { return (uint64_t)a < k; });
        const uint64_t t = it != u.add_pos.end() ? u.add_time[it - u.add_pos.begin()] : u.flush_time;
        v.push_back(Emitted{&c, t, false, u.buffer == 0});
    }
    std::stable_sort(v.begin(), v.end(), [](const Emitted &a, const Emitted &b) {
        if (a.close_time != b.close_time) return a.close_time < b.close_time;
        return a.c->r.left < b.c->r.left;
    });
    // Q2: the reverse buffer's first candidate keeps the ctor's forward label
    for (Emitted &e : v)
        if (out.units[e.c->unit_index].buffer == 1) {
            e.forward_label = true;
            break;
        }
    for (Emitted &e : v) e.written = e.c->r.accepted && e.close_time <= last_write;  // Q3
    if (accepted_only) {
        std::vector<Emitted> a;
        for (const Emitted &e : v)
            if (e.c->r.accepted) a.push_back(e);
        return a;
    }
    return v;
}

// per device: the positions of `regs` it holds (its local candidate
// indices); one hash of the device's candidate list instead of a search per
// region
static void device_regions(const PassResult &out, const DeviceJob &job,
                           const std::vector<const Candidate *> &regs, std::vector<uint64_t> &idx,
                           std::vector<size_t> &where) {
    std::unordered_map<uint64_t, uint64_t> local;
    local.reserve(job.cand_idx.size() * 2);
    for (size_t i = 0; i < job.cand_idx.size(); ++i) local.emplace(job.cand_idx[i], (uint64_t)i);
    idx.clear();
    where.clear();
    for (size_t k = 0; k < regs.size(); ++k) {
        auto it = local.find((uint64_t)(regs[k] - out.cands.data()));
        if (it == local.end()) continue;
        idx.push_back(it->second);
        where.push_back(k);
    }
}

void shift_scan(const EngineParams &ep, PassResult &out, const std::vector<const Candidate *> &regs,
                uint16_t max_shift, std::vector<double> &table) {
    (void)ep;
    const size_t W = (size_t)max_shift + 1;
    table.assign(regs.size() * W, 0.0);
    std::vector<uint64_t> idx;
    std::vector<size_t> where;
    for (DeviceJob &job : g_jobs) {
        if (!job.ctx) continue;
        device_regions(out, job, regs, idx, where);
        if (idx.empty()) continue;
        std::vector<double> t(idx.size() * W);
        check(up_shift_scan(job.ctx, idx.data(), idx.size(), max_shift, t.data()), "up_shift_scan");
        for (size_t j = 0; j < idx.size(); ++j)
            std::copy(t.begin() + j * W, t.begin() + (j + 1) * W, table.begin() + where[j] * W);
    }
}

void shift_best(const EngineParams &ep, PassResult &out, const std::vector<const Candidate *> &regs,
                uint16_t max_shift, std::vector<uint16_t> &best, std::vector<double> &best_corr) {
    (void)ep;
    best.assign(regs.size(), 0);
    best_corr.assign(regs.size(), -1.0);
    std::vector<uint64_t> idx;
    std::vector<size_t> where;
    for (DeviceJob &job : g_jobs) {
        if (!job.ctx) continue;
        device_regions(out, job, regs, idx, where);
        if (idx.empty()) continue;
        std::vector<uint16_t> b(idx.size());
        std::vector<double> c(idx.size());
        check(up_shift_best(job.ctx, idx.data(), idx.size(), max_shift, b.data(), c.data()), "up_shift_best");
        for (size_t j = 0; j < idx.size(); ++j) {
            best[where[j]] = b[j];
            best_corr[where[j]] = c[j];
        }
    }
}

void ProfileSink::header() {  // FormatOutStream::trackHeader, format.cpp:1164-1219
    std::fprintf(fp, "track name=\"%s", name.c_str());
    if (directional) std::fputs(forward ? " +" : " -", fp);
    std::fputc('"', fp);
    if (directional) std::fprintf(fp, " description=\"%s\"", forward ? name.c_str() : " ");
    std::fputs(" priority=2 visibility=", fp);  // PROFILE_PRIORITY, defaults.hpp:42
    if (directional)
        std::fputs(forward ? "full type=wiggle_0 alwaysZero=on color=0,0,255"
                           : "full type=wiggle_0 alwaysZero=on color=255,0,0 altColor=255,0,0", fp);
    else
        std::fputs("full type=wiggle_0 alwaysZero=on color=191,0,191", fp);
    if (!assembly.empty()) std::fprintf(fp, " db=%s", assembly.c_str());
    std::fputc('\n', fp);
}

void ProfileSink::start_line(bool fwd, uint32_t c) {
    if (directional) {
        if (!have_contig || forward != fwd) {
            forward = fwd;
            have_contig = false;
            header();
        }
    } else if (!have_contig) {
        header();
    }
    if (!have_contig || contig != c) {
        contig = c;
        have_contig = true;
        std::fprintf(fp, "variableStep chrom=%s\n", ct->name(c).c_str());
    }
}

void ProfileSink::write(bool fwd, uint32_t c, uint64_t pos, double score) {
    if (score == 0) return;  // format.cpp:1092
    start_line(fwd, c);
    ++stats.host_lines;
    // ostream << double: 6 significant digits (%g); reverse strand negated
    std::fprintf(fp, (directional && !fwd) ? "%llu -%g\n" : "%llu %g\n", (unsigned long long)pos, score);
}

void ProfileSink::write_block(bool fwd, uint32_t c, const char *text, size_t n) {
    if (!n) return;  // the reference switches headers only when it writes a line
    start_line(fwd, c);
    if (std::fwrite(text, 1, n, fp) != n) fatal("-w: short write of the profile");
}

void write_profile(const PassResult &pr, uint16_t bw, ProfileSink &sink) {
    // device context and unit id of every global unit
    std::vector<std::pair<up_ctx *, uint32_t>> where(pr.units.size(), {nullptr, 0});
    for (const DeviceJob &j : g_jobs)
        for (size_t k = 0; k < j.dev_unit.size(); ++k) where[j.dev_unit[k]] = {j.ctx, (uint32_t)k};
    // Units the exact replay produced (quirk Q1 heads, -r <= 0, bw > 255)
    // hand over their retirements as the state machine wrote them: every
    // nonzero (pos, score) with the add() -- or flush -- whose retirement loop
    // wrote it.  Positions at or after a resync point follow the dense KDE.
    struct Replayed { uint32_t resync = 0; std::vector<uint32_t> event, pos; std::vector<double> score; };
    std::vector<Replayed> rep(pr.units.size());
    for (uint32_t k = 0; k < pr.units.size(); ++k) {
        Replayed &r = rep[k];
        uint64_t n = 0;
        int rc = up_unit_replay_profile(where[k].first, where[k].second, &r.resync, &n, nullptr, nullptr,
                                        nullptr, 0);
        if (rc != UP_OK) fatal(std::string("up_unit_replay_profile: ") + up_strerror(rc));
        r.event.resize(n);
        r.pos.resize(n);
        r.score.resize(n);
        if (n && (rc = up_unit_replay_profile(where[k].first, where[k].second, &r.resync, &n, r.event.data(),
                                              r.pos.data(), r.score.data(), n)) != UP_OK)
            fatal(std::string("up_unit_replay_profile: ") + up_strerror(rc));
    }
    // retirement events in the driver's call order: add() at p after q retires
    // q-bw .. q-bw+min(W,p-q)-1 (peakcall.cpp:171-184); flushContig()
    // retires q-bw .. q+bw.  A replayed unit's entries go out at the event
    // that wrote them, before the dense positions of the same event.
    struct Ev { uint64_t t; uint32_t unit; int kind; int64_t lo, hi; };  // kind 0: replayed [lo, hi) entries
    std::vector<Ev> ev;
    const int64_t W = 2 * (int64_t)bw + 1;
    for (uint32_t k = 0; k < pr.units.size(); ++k) {
        const UnitBuild &u = pr.units[k];
        const Replayed &r = rep[k];
        for (size_t i = 0; i < r.event.size();) {  // runs of one event
            size_t j = i;
            while (j < r.event.size() && r.event[j] == r.event[i]) ++j;
            const uint32_t e = r.event[i];
            uint64_t t;
            if (e == UP_FLUSH_EVENT) t = u.flush_time;
            else if (e < u.add_time.size()) t = u.add_time[e];
            else fatal("-w: the replay's add index exceeds the unit's adds");
            ev.push_back({t, k, 0, (int64_t)i, (int64_t)j});
            i = j;
        }
        if (r.resync == UP_FLUSH_EVENT) continue;  // replayed to the end
        const int64_t x0 = r.resync ? (int64_t)r.resync : 1;  // dense from the resync point on
        int64_t q = 0;
        for (size_t i = 0; i < u.add_pos.size(); ++i) {
            const int64_t p = u.add_pos[i];
            if (q != 0 && p > q) {
                const int64_t n = std::min<int64_t>(W, p - q);
                const int64_t lo = std::max<int64_t>({1, q - bw, x0}), hi = q - bw + n - 1;
                if (lo <= hi) ev.push_back({u.add_time[i], k, 1, lo, hi});
            }
            q = p;
        }
        if (q != 0) {
            const int64_t lo = std::max<int64_t>({1, q - bw, x0}), hi = q + bw;
            if (lo <= hi) ev.push_back({u.flush_time, k, 1, lo, hi});
        }
    }
    std::stable_sort(ev.begin(), ev.end(), [](const Ev &a, const Ev &b) {
        return a.t != b.t ? a.t < b.t : a.kind < b.kind;
    });
    // One chunk of a unit's dense profile at a time, chunk-aligned.  By default
    // the device formats the chunk's lines itself (up_unit_profile_text) and
    // the host only slices that text; a chunk the device does not format
    // exactly (exact = 0), a refused call and UNIPEAK_PROFILE_TEXT=0 keep the
    // scores and sink.write().
    uint32_t chunk_pos = 1u << 22;
    if (const char *e = std::getenv("UNIPEAK_PROFILE_TEXT_CHUNK")) {  // tests: slices across chunk edges
        const unsigned long long v = std::strtoull(e, nullptr, 10);
        if (v >= 64 && v <= (1ull << 30)) chunk_pos = (uint32_t)v;
    }
    const char *et = std::getenv("UNIPEAK_PROFILE_TEXT");
    const bool use_text = !(et && et[0] == '0');
    // A maximal run of time-consecutive dense events of one unit is one slice
    // [lo, hi): a unit's events are ascending and disjoint and the positions
    // between them have no tag within bw, so no line; the concatenation of a
    // unit's slices is its text.  The slice ends are the cuts of their chunks.
    struct Slice { uint32_t unit; int64_t lo, hi; };
    std::vector<Slice> slices;  // in emission order; kind-0 events keep their place through `at`
    std::vector<size_t> at(ev.size(), ~(size_t)0);  // event -> the slice it starts (kind 1), else none
    std::vector<std::vector<uint64_t>> cuts(pr.units.size());
    for (size_t i = 0; i < ev.size();) {
        if (ev[i].kind == 0) {
            ++i;
            continue;
        }
        size_t j = i;
        while (j + 1 < ev.size() && ev[j + 1].kind == 1 && ev[j + 1].unit == ev[i].unit) ++j;
        at[i] = slices.size();
        slices.push_back({ev[i].unit, ev[i].lo, ev[j].hi + 1});
        cuts[ev[i].unit].push_back((uint64_t)ev[i].lo);
        cuts[ev[i].unit].push_back((uint64_t)ev[j].hi + 1);
        i = j + 1;
    }
    struct Cache {
        int64_t first = -1;
        uint32_t n = 0;
        bool text = false;
        std::string bytes;                  // text: the chunk's lines
        std::vector<uint64_t> cpos, coff;   // text: its cuts and their byte offsets
        std::vector<double> f, r;           // else: its scores
    };
    std::vector<Cache> cache(pr.units.size());
    ProfileStats &st = sink.stats;
    auto load = [&](uint32_t unit, int64_t x) {  // the chunk that holds position x
        Cache &c = cache[unit];
        const UnitBuild &u = pr.units[unit];
        c.first = ((x - 1) / chunk_pos) * (int64_t)chunk_pos + 1;
        const uint64_t dom_end = (uint64_t)u.len + bw;  // highest position a flush retires
        c.n = (uint64_t)c.first > dom_end
                  ? 0 : (uint32_t)std::min<uint64_t>(chunk_pos, dom_end - (uint64_t)c.first + 1);
        c.text = false;
        if (!c.n) return;  // beyond the scan domain: never scored
        ++st.chunks;
        if (use_text) {
            const std::vector<uint64_t> &all = cuts[unit];
            const auto a = std::lower_bound(all.begin(), all.end(), (uint64_t)c.first);
            const auto b = std::upper_bound(all.begin(), all.end(), (uint64_t)c.first + c.n);
            c.cpos.assign(a, b);
            c.coff.assign(c.cpos.size(), 0);
            const char *text = nullptr;
            uint64_t nb = 0, nl = 0;
            int32_t exact = 0;
            const int rc = up_unit_profile_text(where[unit].first, where[unit].second, (uint64_t)c.first, c.n,
                                                sink.directional && u.buffer != 0, (uint32_t)c.cpos.size(),
                                                c.cpos.data(), c.coff.data(), &text, &nb, &nl, &exact);
            if (rc == UP_OK) {
                double ms[9] = {0};
                if (up_timings(where[unit].first, ms, 9) == UP_OK) {
                    st.dense_ms += ms[5];
                    st.text_ms += ms[8];
                }
            }
            if (rc == UP_OK && exact) {
                c.text = true;
                c.bytes.assign(text ? text : "", nb);
                st.device_bytes += nb;
                st.device_lines += nl;
                return;
            }
            ++st.fallback_chunks;
        }
        c.f.assign(c.n, 0.0);
        c.r.assign(c.n, 0.0);
        const int rc = up_unit_profile_range(where[unit].first, where[unit].second, (uint64_t)c.first, c.n,
                                             c.f.data(), c.r.data());
        if (rc != UP_OK) fatal(std::string("up_unit_profile_range: ") + up_strerror(rc));
        double ms[6] = {0};
        if (up_timings(where[unit].first, ms, 6) == UP_OK) st.dense_ms += ms[5];
    };
    auto offset_of = [](const Cache &c, uint64_t x) -> uint64_t {  // bytes of the chunk's lines below x
        if (x == (uint64_t)c.first) return 0;
        if (x == (uint64_t)c.first + c.n) return c.bytes.size();
        const auto it = std::lower_bound(c.cpos.begin(), c.cpos.end(), x);
        if (it == c.cpos.end() || *it != x) fatal("-w: a slice end is not among its chunk's cuts");
        return c.coff[it - c.cpos.begin()];
    };
    for (size_t i = 0; i < ev.size(); ++i) {
        const Ev &e = ev[i];
        const UnitBuild &u = pr.units[e.unit];
        if (e.kind == 0) {
            const Replayed &r = rep[e.unit];
            for (int64_t k = e.lo; k < e.hi; ++k) sink.write(u.buffer == 0, u.contig, r.pos[k], r.score[k]);
            continue;
        }
        if (at[i] == ~(size_t)0) continue;  // inside a slice already written
        const Slice &sl = slices[at[i]];
        Cache &c = cache[e.unit];
        for (int64_t x = sl.lo; x < sl.hi;) {
            if (c.first < 0 || x < c.first || x >= c.first + (int64_t)chunk_pos) load(e.unit, x);
            const int64_t end = std::min<int64_t>(sl.hi, c.first + (int64_t)c.n);
            if (end <= x) break;  // beyond the scan domain: never scored
            if (c.text) {
                const uint64_t o0 = offset_of(c, (uint64_t)x), o1 = offset_of(c, (uint64_t)end);
                sink.write_block(u.buffer == 0, u.contig, c.bytes.data() + o0, o1 - o0);
            } else {
                for (int64_t y = x; y < end; ++y) {
                    const size_t k = (size_t)(y - c.first);
                    sink.write(u.buffer == 0, u.contig, (uint64_t)y, c.f[k] + c.r[k]);
                }
            }
            x = end;
        }
    }
}

namespace {

static_assert(sizeof(up_bw_item) == 8 && sizeof(up_bw_zoom) == sizeof(bbi::ZoomRecord),
              "items and zoom records go to disk as the device wrote them");

// what wigs2bigwigs makes of the -w line of `score`: the text's double, cast
// to float; the reverse buffer's line carries a '-' in front of the %g text
float bw_host_value(double score, bool negate) {
    float f = 0;
    int ok = 0;
    if (!(negate && score < 0) && up_g6_to_float(score, &f, &ok) == UP_OK && ok) return negate ? -f : f;
    char buf[64];
    std::snprintf(buf, sizeof buf, negate ? "-%g" : "%g", score);
    return (float)std::strtod(buf, nullptr);
}

up_bw_section bw_host_section(const up_bw_item *it, size_t n) {
    up_bw_section s{};
    s.start = it[0].start;
    s.end = it[n - 1].start + 1;
    s.count = (uint32_t)n;
    s.vmin = s.vmax = it[0].value;
    for (size_t i = 0; i < n; ++i) {
        const double v = it[i].value;
        s.vmin = std::min(s.vmin, it[i].value);
        s.vmax = std::max(s.vmax, it[i].value);
        s.sum += v;
        s.sumsq += v * v;
    }
    return s;
}

// the zoom records of sorted items on the fixed grid, level by level
void bw_host_zoom(const std::vector<up_bw_item> &items, uint32_t chrom, uint32_t clip_end, uint32_t red0,
                  uint32_t n_levels, std::vector<std::vector<up_bw_zoom>> &zoom) {
    uint64_t red = red0;
    for (uint32_t z = 0; z < n_levels; ++z, red *= 4) {
        for (size_t i = 0; i < items.size();) {
            const uint64_t bin = items[i].start / red;
            up_bw_zoom r{};
            r.chrom = chrom;
            r.start = (uint32_t)(bin * red);
            r.end = (uint32_t)std::min<uint64_t>(bin * red + red, clip_end);
            r.vmin = r.vmax = items[i].value;
            double sum = 0, sumsq = 0;
            for (; i < items.size() && items[i].start / red == bin; ++i) {
                const double v = items[i].value;
                r.vmin = std::min(r.vmin, items[i].value);
                r.vmax = std::max(r.vmax, items[i].value);
                sum += v;
                sumsq += v * v;
                ++r.valid;
            }
            r.sum = (float)sum;
            r.sumsq = (float)sumsq;
            zoom[z].push_back(r);
        }
    }
}

// one bigWig file being written: data sections are appended as they come,
// the index and the zoom records wait for the trailer
struct BwTrack {
    std::string path;
    std::FILE *fp = nullptr;
    uint64_t at = 0;  // file offset
    uint64_t summary_off = 0, tree_off = 0, data_off = 0;
    std::vector<std::string> names;  // chromosomes that hold items, in id order
    std::vector<uint32_t> sizes;
    std::vector<bbi::Block> blocks;
    std::vector<std::vector<up_bw_zoom>> zoom;
    uint32_t red0 = 10, max_raw = 0;
    uint64_t valid = 0, nitems = 0;
    double vmin = 0, vmax = 0, sum = 0, sumsq = 0;

    void put(const std::string &s) {
        if (std::fwrite(s.data(), 1, s.size(), fp) != s.size()) fatal("-W: short write of " + path);
        at += s.size();
    }
    void open(size_t max_chroms, size_t max_key, uint32_t n_levels) {
        fp = std::fopen(path.c_str(), "wb");
        if (!fp) fatal("could not write " + path);
        std::setvbuf(fp, nullptr, _IOFBF, 1 << 22);
        zoom.assign(n_levels, {});
        // header, zoom headers, total summary and chromosome tree are written by
        // finish(); the tree's room is that of every contig the track may hold
        summary_off = bbi::kHeaderBytes + bbi::kZoomHeaderBytes * n_levels;
        tree_off = summary_off + bbi::kSummaryBytes;
        data_off = tree_off + bbi::chrom_tree_bytes(max_chroms, std::max<size_t>(1, max_key));
        put(std::string(data_off + 8, '\0'));  // + the section count
    }
    // the sections of n items of one chunk (sec: their records, or null), compressed on T threads
    bbi::DeviceDeflater *dev = nullptr;  // UNIPEAK_BIGWIG_DEFLATE=device: sections and zoom blocks go through it
    void add_sections(uint32_t chrom, const up_bw_item *it, size_t n, const up_bw_section *sec, unsigned T,
                      BigWigStats &st) {
        if (!n) return;
        const size_t nsec = (n + bbi::kItemsPerSection - 1) / bbi::kItemsPerSection;
        std::vector<std::string> comp(nsec);
        std::vector<up_bw_section> rec(nsec);
        std::atomic<size_t> next{0};
        std::atomic<bool> failed{false};
        // the device's encoder: every section's header and items in one buffer, one call
        auto on_device = [&] {
            std::string raw;
            raw.reserve(n * sizeof(up_bw_item) + nsec * bbi::kSectionHeaderBytes);
            std::vector<uint64_t> off(nsec + 1, 0);
            for (size_t s = 0; s < nsec; ++s) {
                const up_bw_item *a = it + s * bbi::kItemsPerSection;
                const size_t k = std::min<size_t>(bbi::kItemsPerSection, n - s * bbi::kItemsPerSection);
                rec[s] = sec ? sec[s] : bw_host_section(a, k);
                bbi::put_section_header(raw, chrom, rec[s].start, rec[s].end, 1, (uint16_t)k);
                raw.append((const char *)a, k * sizeof(up_bw_item));
                off[s + 1] = raw.size();
            }
            if (!dev->segments(raw.data(), off, comp)) failed = true;
        };
        auto work = [&] {
            std::string raw;
            for (size_t s; (s = next.fetch_add(1)) < nsec;) {
                const up_bw_item *a = it + s * bbi::kItemsPerSection;
                const size_t k = std::min<size_t>(bbi::kItemsPerSection, n - s * bbi::kItemsPerSection);
                rec[s] = sec ? sec[s] : bw_host_section(a, k);
                raw.clear();
                bbi::put_section_header(raw, chrom, rec[s].start, rec[s].end, 1, (uint16_t)k);
                raw.append((const char *)a, k * sizeof(up_bw_item));
                if (!bbi::deflate6(raw.data(), raw.size(), comp[s])) failed = true;
            }
        };
        const auto t0 = std::chrono::steady_clock::now();
        const unsigned nt = (unsigned)std::min<size_t>(T, nsec);
        if (dev) {
            on_device();
        } else if (nt <= 1) {
            work();
        } else {
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < nt; ++t) pool.emplace_back(work);
            for (auto &th : pool) th.join();
        }
        st.compress_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (failed) fatal("-W: compression failed");
        for (size_t s = 0; s < nsec; ++s) {
            const up_bw_section &r = rec[s];
            max_raw = std::max<uint32_t>(max_raw, (uint32_t)(bbi::kSectionHeaderBytes + r.count * sizeof(up_bw_item)));
            blocks.push_back(bbi::Block{chrom, r.start, r.end, at, comp[s].size()});
            put(comp[s]);
            vmin = valid ? std::min<double>(vmin, r.vmin) : r.vmin;
            vmax = valid ? std::max<double>(vmax, r.vmax) : r.vmax;
            valid += r.count;
            sum += r.sum;
            sumsq += r.sumsq;
        }
        nitems += n;
        st.sections += nsec;
    }
    void finish(unsigned T, BigWigStats &st) {
        const auto t0 = std::chrono::steady_clock::now();
        if (!nitems) {  // no line, no track header in the -w file: wigs2bigwigs writes no file
            std::fclose(fp);
            fp = nullptr;
            std::remove(path.c_str());
            return;
        }
        const uint64_t index_off = at;
        std::string f;
        bbi::write_rtree(f, blocks, bbi::kRtreeBlock, bbi::kItemsPerSection, at);
        put(f);
        // a level is kept while it has fewer records than the one before it
        // (and than the items): wigs2bigwigs's rule
        std::vector<bbi::ZoomPlace> places;
        uint64_t prev = nitems, red = red0;
        for (size_t z = 0; z < zoom.size(); ++z, red *= 4) {
            if (zoom[z].empty() || zoom[z].size() >= prev) break;
            prev = zoom[z].size();
            f.clear();
            bbi::ZoomPlace place{};
            if (!bbi::write_zoom_level(f, (const bbi::ZoomRecord *)zoom[z].data(), zoom[z].size(), (uint32_t)red,
                                       max_raw, place, at, T, dev))
                fatal("-W: compression failed");
            put(f);
            places.push_back(place);
        }
        f.clear();
        bbi::put32(f, bbi::kMagic);
        put(f);
        std::string head = bbi::header_bytes(tree_off, data_off, index_off, summary_off, max_raw, places);
        head.resize(summary_off, '\0');
        head += bbi::summary_bytes(valid, vmin, vmax, sum, sumsq);
        bbi::write_chrom_tree(head, names, sizes);
        if (head.size() > data_off) fatal("-W: the chromosome tree outgrew its room");
        head.resize(data_off, '\0');
        bbi::put64(head, blocks.size());
        if (std::fseek(fp, 0, SEEK_SET) != 0 || std::fwrite(head.data(), 1, head.size(), fp) != head.size() ||
            std::fclose(fp) != 0)
            fatal("-W: could not finish " + path);
        fp = nullptr;
        st.trailer_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
};

}  // namespace

void write_profile_bigwig(const PassResult &pr, uint16_t bw, BigWigSink &sink) {
    (void)bw;
    const ContigTable &ct = *sink.ct;
    BigWigStats &st = sink.stats;
    std::vector<std::pair<up_ctx *, uint32_t>> where(pr.units.size(), {nullptr, 0});
    for (const DeviceJob &j : g_jobs)
        for (size_t k = 0; k < j.dev_unit.size(); ++k) where[j.dev_unit[k]] = {j.ctx, (uint32_t)k};
    // a chunk is a multiple of the top level's bin, so no bin of any level
    // straddles two calls: 10 * 4^9 positions, ten levels from 10 bases up
    const uint32_t red0 = 10;
    uint64_t chunk = (uint64_t)red0 << 18;
    uint32_t n_levels = UP_BW_MAX_LEVELS;
    if (const char *e = std::getenv("UNIPEAK_BIGWIG_CHUNK")) {  // tests: several chunks of a short contig
        const unsigned long long v = std::strtoull(e, nullptr, 10);
        if (v >= 1 && v <= (1ull << 30)) {
            chunk = v;
            n_levels = 0;  // as many levels as keep the chunk a multiple of the top bin
            for (uint64_t r = red0; n_levels < UP_BW_MAX_LEVELS && chunk % r == 0; r *= 4) ++n_levels;
        }
    }
    const unsigned T = std::min(16u, ingest_threads());
    // the units of each track, by contig: one unit per contig
    const int ntracks = sink.directional ? 2 : 1;
    std::vector<std::vector<uint32_t>> units(ntracks);
    for (int b = 0; b < ntracks; ++b) {
        std::vector<int64_t> seen(ct.size(), -1);
        for (uint32_t k = 0; k < pr.units.size(); ++k) {
            const UnitBuild &u = pr.units[k];
            if (u.buffer != b) continue;
            if (seen[u.contig] >= 0)
                fatal("-W: contig " + ct.name(u.contig) + " reaches the " +
                      (sink.directional ? (b ? "reverse" : "forward") : "only") +
                      " track from more than one unit (its records are interleaved with another contig's); "
                      "a bigWig cannot hold overlapping items");
            seen[u.contig] = k;
            units[b].push_back(k);
        }
        std::stable_sort(units[b].begin(), units[b].end(), [&](uint32_t x, uint32_t y) {
            return ct.name(pr.units[x].contig) < ct.name(pr.units[y].contig);
        });
    }
    bbi::DeviceDeflater deflater;
    const bool on_device = bbi::DeviceDeflater::wanted();
    for (int b = 0; b < ntracks; ++b) {
        BwTrack t;
        if (on_device) t.dev = &deflater;
        t.path = sink.root + (sink.directional ? (b ? "-" : "+") : "") + ".bw";
        t.red0 = red0;
        if (units[b].size() > 65535) fatal("-W: too many chromosomes for one B+ tree node");
        size_t max_key = 1;
        for (uint32_t k : units[b]) max_key = std::max(max_key, ct.name(pr.units[k].contig).size());
        t.open(units[b].size(), max_key, n_levels);
        const bool negate = sink.directional && b != 0;
        for (uint32_t k : units[b]) {
            const UnitBuild &u = pr.units[k];
            up_ctx *ctx = where[k].first;
            const uint32_t du = where[k].second;
            const uint32_t chrom = (uint32_t)t.names.size();  // its id once it holds an item
            const uint64_t before = t.nitems;
            std::vector<size_t> z0(n_levels);  // where the unit's zoom records start
            for (uint32_t z = 0; z < n_levels; ++z) z0[z] = t.zoom[z].size();
            // replayed entries: converted on the host, the unit's first sections
            uint32_t resync = 0;
            uint64_t n = 0;
            int rc = up_unit_replay_profile(ctx, du, &resync, &n, nullptr, nullptr, nullptr, 0);
            if (rc != UP_OK) fatal(std::string("up_unit_replay_profile: ") + up_strerror(rc));
            std::vector<up_bw_item> head;  // items the host zoom sees: replayed, then the resync chunk's
            if (n) {
                std::vector<uint32_t> ev(n), pos(n);
                std::vector<double> score(n);
                if ((rc = up_unit_replay_profile(ctx, du, &resync, &n, ev.data(), pos.data(), score.data(), n)) != UP_OK)
                    fatal(std::string("up_unit_replay_profile: ") + up_strerror(rc));
                for (uint64_t i = 0; i < n; ++i) {
                    if (score[i] == 0 || pos[i] > u.len) continue;  // no line; -clip
                    if (pos[i] == 0) fatal("-W: a replayed entry at position 0");
                    head.push_back(up_bw_item{pos[i] - 1, bw_host_value(score[i], negate)});
                }
                std::stable_sort(head.begin(), head.end(),
                                 [](const up_bw_item &x, const up_bw_item &y) { return x.start < y.start; });
                st.host_items += head.size();
                t.add_sections(chrom, head.data(), head.size(), nullptr, T, st);
            }
            const bool replayed_part = resync != 0;
            if (resync != UP_FLUSH_EVENT) {
                const uint64_t x0 = resync ? resync : 1;  // dense from the resync point on
                for (uint64_t first = ((x0 - 1) / chunk) * chunk + 1; first <= u.len; first += chunk) {
                    const uint32_t count = (uint32_t)std::min<uint64_t>(chunk, (uint64_t)u.len - first + 1);
                    ++st.chunks;
                    const up_bw_item *items = nullptr;
                    const up_bw_section *secs = nullptr;
                    const up_bw_zoom *zp[UP_BW_MAX_LEVELS] = {nullptr};
                    uint64_t ni = 0, ns = 0, zn[UP_BW_MAX_LEVELS] = {0};
                    int32_t exact = 0;
                    rc = up_unit_profile_bigwig(ctx, du, first, count, negate, u.len, red0, n_levels, chrom, &items,
                                                &ni, &secs, &ns, zp, zn, &exact);
                    if (rc != UP_OK) fatal(std::string("up_unit_profile_bigwig: ") + up_strerror(rc));
                    double ms[10] = {0};
                    if (up_timings(ctx, ms, 10) == UP_OK) {
                        st.dense_ms += ms[5];
                        st.bigwig_ms += ms[9];
                    }
                    const bool cut = first < x0;  // the chunk that holds resync: positions below it are dropped
                    if (exact && !cut) {
                        st.device_items += ni;
                        t.add_sections(chrom, items, ni, secs, T, st);
                        for (uint32_t z = 0; z < n_levels; ++z) t.zoom[z].insert(t.zoom[z].end(), zp[z], zp[z] + zn[z]);
                        continue;
                    }
                    std::vector<up_bw_item> own;
                    if (exact) {
                        const up_bw_item *a = std::lower_bound(
                            items, items + ni, (uint32_t)(x0 - 1),
                            [](const up_bw_item &x, uint32_t s) { return x.start < s; });
                        own.assign(a, items + ni);
                        st.device_items += own.size();
                    } else {  // converted on the host from the scores
                        ++st.fallback_chunks;
                        std::vector<double> f(count, 0.0), r(count, 0.0);
                        rc = up_unit_profile_range(ctx, du, first, count, f.data(), r.data());
                        if (rc != UP_OK) fatal(std::string("up_unit_profile_range: ") + up_strerror(rc));
                        if (up_timings(ctx, ms, 6) == UP_OK) st.dense_ms += ms[5];
                        for (uint64_t i = (cut ? x0 - first : 0); i < count; ++i) {
                            const double s = f[i] + r[i];
                            if (s != 0) own.push_back(up_bw_item{(uint32_t)(first + i - 1), bw_host_value(s, negate)});
                        }
                        st.host_items += own.size();
                    }
                    t.add_sections(chrom, own.data(), own.size(), nullptr, T, st);
                    if (cut) {  // its bins are summarised with the replayed part's, below
                        head.insert(head.end(), own.begin(), own.end());
                    } else {
                        bw_host_zoom(own, chrom, u.len, red0, n_levels, t.zoom);
                    }
                }
            }
            if (replayed_part) {
                // (the cut chunk's zoom has to come before the later chunks': levels are in start order)
                std::vector<std::vector<up_bw_zoom>> hz(n_levels);
                bw_host_zoom(head, chrom, u.len, red0, n_levels, hz);
                for (uint32_t z = 0; z < n_levels; ++z) {
                    auto &dst = t.zoom[z];
                    dst.insert(dst.begin() + (std::ptrdiff_t)z0[z], hz[z].begin(), hz[z].end());
                }
            }
            if (t.nitems != before) {
                t.names.push_back(ct.name(u.contig));
                t.sizes.push_back(u.len);
            }
        }
        t.finish(T, st);
    }
    st.deflate_device = on_device;
    st.deflate_ms = deflater.device_ms();
}

void release_devices() {
    join_prewarm();
    for (DeviceJob &j : g_jobs)
        if (j.ctx) up_close(j.ctx);
    g_jobs.clear();
    for (up_ctx *c : g_pre)
        if (c) up_close(c);
    g_pre.clear();
}

}  // namespace unipeak
