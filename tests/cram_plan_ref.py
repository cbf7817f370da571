"""A plain sequential reading of the device plan of a CRAM's quality blocks (the layout NGSQC_CRAM_PLAN_DUMP writes: csrc/cram_plan.h): the reference the kernels of
csrc/cram_dev_kernels.h are held against. It knows nothing of lanes: one state after the other, a linear search through the cumulative row, renormalisation byte by
byte - hts-specs CRAMcodecs, rANS 4x8. A plan that does not decode is reported, not asserted: the tests hand in damaged plans as well."""
import struct

JOB = struct.Struct("<QQIIIIII")      # in_off, out_off, in_len, n_out, tab_off, sym_off, order, nsym
PATCH = struct.Struct("<QQII")        # dst, src, len, pad
ST_JOB, ST_STREAM, ST_SRC, ST_DST = 1, 2, 4, 8   # the kernels' status bits


class Plan:
    def __init__(self, jobs, tabs, syms, patches, out_bytes):
        self.jobs, self.tabs, self.syms, self.patches, self.out_bytes = jobs, tabs, syms, patches, out_bytes

    def copy(self):
        return Plan([list(j) for j in self.jobs], list(self.tabs), bytearray(self.syms), [list(p) for p in self.patches], self.out_bytes)


def load_plan(path):
    d = open(path, "rb").read()
    nj, nt, ns_, npch, out_bytes = struct.unpack_from("<5Q", d, 0); o = 40
    jobs = [list(JOB.unpack_from(d, o + 40 * i)) for i in range(nj)]; o += 40 * nj
    tabs = list(struct.unpack_from("<%dH" % nt, d, o)); o += 2 * nt
    syms = bytearray(d[o:o + ns_]); o += ns_
    patches = [list(PATCH.unpack_from(d, o + 24 * i)) for i in range(npch)]
    return Plan(jobs, tabs, syms, patches, out_bytes)


class Bad(Exception):
    pass


def decode_job(plan, job, cram):
    """-> (status bit or 0, decoded bytes, facts): facts = what the block exercised (for the tables of reached cases)"""
    in_off, out_off, in_len, n_out, tab_off, sym_off, order, ns = job
    facts = dict(min_f=4096, max_f=0, max_two=0, two=0, zero_row=False, one_successor=False)
    if in_len < 16 or ns < 1 or ns > 64: return ST_JOB, None, facts
    tabs = plan.tabs; sym = plan.syms[sym_off:sym_off + 64]; row = ns + 1; end = in_off + in_len
    R = list(struct.unpack_from("<4I", cram, in_off)); p = in_off + 16; out = bytearray(n_out)
    if order:
        for r in range(ns):
            C = tabs[tab_off + r * row:tab_off + (r + 1) * row]
            if C[ns] == 0: facts["zero_row"] = True
            elif sum(1 for k in range(ns) if C[k + 1] > C[k]) == 1: facts["one_successor"] = True

    def step(j, C0):
        nonlocal p
        x = R[j]; m = x & 0xfff; k = 0
        while k + 1 < ns and tabs[C0 + k + 1] <= m: k += 1
        c0 = tabs[C0 + k]; f = tabs[C0 + k + 1] - c0
        if f <= 0 or not c0 <= m < c0 + f: raise Bad()
        if f < facts["min_f"]: facts["min_f"] = f
        if f > facts["max_f"]: facts["max_f"] = f
        v = (f * (x >> 12) + m - c0) & 0xffffffff; cnt = 0   # (32-bit states, as every decoder of the format keeps them)
        while v < (1 << 23):
            if p >= end: raise Bad()
            v = (v << 8) | cram[p]; p += 1; cnt += 1
        R[j] = v
        return k, cnt
    try:
        if order == 0:
            for i in range(0, n_out, 4):
                two = 0
                for j in range(min(4, n_out - i)):
                    k, cnt = step(j, tab_off); out[i + j] = sym[k]; two += cnt == 2
                if two:
                    facts["two"] += 1
                    if two > facts["max_two"]: facts["max_two"] = two
        else:
            q = n_out >> 2; idx = [0, q, 2 * q, 3 * q]; k0 = plan.syms[sym_off + 64]
            if k0 >= ns: raise Bad()
            pk = [k0] * 4
            for _ in range(q):
                two = 0
                for j in range(4):
                    k, cnt = step(j, tab_off + pk[j] * row); out[idx[j]] = sym[k]; idx[j] += 1; pk[j] = k; two += cnt == 2
                if two:
                    facts["two"] += 1
                    if two > facts["max_two"]: facts["max_two"] = two
            while idx[3] < n_out:
                k, _ = step(3, tab_off + pk[3] * row); out[idx[3]] = sym[k]; idx[3] += 1; pk[3] = k
    except Bad:
        return ST_STREAM, None, facts
    return 0, bytes(out), facts


def decode_jobs(plan, cram):
    """-> [(status, bytes | None, facts)] per job"""
    return [decode_job(plan, j, cram) for j in plan.jobs]


def patch_stream(plan, qs, stream, image_bytes=None):
    """the second kernel, sequentially: -> (status, stream). A patch that reaches behind the decoded bytes is refused as a whole (ST_SRC); one that reaches behind the
    image copies what lies in front of its end (ST_DST)"""
    out = bytearray(stream); status = 0
    for dst, src, ln, _ in plan.patches:
        if src + ln > len(qs): status |= ST_SRC; continue
        if dst + ln <= len(out) and (image_bytes is None or ((dst + ln - 1) // 65280) * 65311 + 23 + (dst + ln - 1) % 65280 < image_bytes): out[dst:dst + ln] = qs[src:src + ln]; continue
        for b in range(ln):
            s = dst + b; at = (s // 65280) * 65311 + 23 + s % 65280
            if (image_bytes is not None and at >= image_bytes) or s >= len(out): status |= ST_DST; break
            out[s] = qs[src + b]
    return status, bytes(out)


def replay_plan(cram_bytes, plan_path, stream):
    """the whole plan on a blank stream -> (stream | None when a block does not decode, jobs, patches)"""
    plan = load_plan(plan_path); qs = bytearray(plan.out_bytes)
    for job, (st, data, _) in zip(plan.jobs, decode_jobs(plan, cram_bytes)):
        if st: return None, len(plan.jobs), len(plan.patches)
        qs[job[1]:job[1] + job[3]] = data
    out = bytearray(stream)
    for dst, src, ln, _ in plan.patches:
        if any(out[dst:dst + ln]) or src + ln > plan.out_bytes: return None, len(plan.jobs), len(plan.patches)
        out[dst:dst + ln] = qs[src:src + ln]
    return bytes(out), len(plan.jobs), len(plan.patches)
