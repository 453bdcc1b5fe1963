"""Any overlay in a handle, with no product change (test infrastructure).

psim_restore checks a snapshot's header and section sizes and then copies the
sections to the device: it trusts their contents.  layout() mirrors the
snapshot's byte layout (SnapHead, the started bytes, then per local shard a
ShardHead and the arrays of snap_sections() in psim_engine.hip, in that order)
as named numpy views over one writable buffer; inject() overwrites in a fresh
snapshot only what a getter reads, restores it and reads the rows back.

The mirror fails loudly: a magic, ABI or config mismatch, or sizes that do not
add up to exactly the snapshot's length, raise LayoutError before anything is
written.  test_gpu_synthetic_overlays.py checks it against nodes() /
strategy_nodes() of real scenarios.

The domain is enforced here, on the host, before any device call: several
getter kernels index by a row's id or run a loop to a row's count without a
bound test, relying on what the engine guarantees.  Next to each field's
validator stands what the getters' kernels assume of it."""
import numpy as np

from partisan_amd import _abi

NONE = 0xFFFFFFFF
MAP_BIT = 0x80000000
CONN_DOWN = 0x80000000
CONN_CLOSING = 0x40000000
F_UP = 1
SNAP_MAGIC = 0x4D495350
RT_SET = _abi.PT_SET_POOL                   # the eager / lazy pool of a node
RT_WORDS = 8                                # PT_ROOTS roots, a word of eager counts, one of lazy counts, 2 spare
IDMAP_IN, OUT_IN = 16, 16
IDMAP_EXT, OUT_EXT = _abi.IDMAP_CAP - IDMAP_IN, _abi.PT_OUT_CAP - OUT_IN
MSG_BYTES = 64

# Hdr of psim_device.h: one 64-B line per node
HDR = np.dtype([("rng", "<u8"), ("start_round", "<u4"), ("join_contact", "<u4"), ("epoch", "<u4"), ("aux", "<u4"),
                ("have", "<u4"), ("trk_round", "<u4"), ("trk_hop", "<u4"),
                ("act_n", "u1"), ("pas_n", "u1"), ("sent_n", "u1"), ("sent_head", "u1"),
                ("recv_n", "u1"), ("recv_head", "u1"), ("all_n", "u1"), ("com_n", "u1"),
                ("conn_n", "u1"), ("conn_dn", "u1"), ("out_n", "u1"), ("conn_cl", "u1"),
                ("pad1", "<u4", (4,))])
SNAP_HEAD = np.dtype([("magic", "<u4"), ("abi", "<u4"), ("n_nodes", "<u4"), ("n_local_shards", "<u4"),
                      ("manager", "<u4"), ("strategy", "<u4"), ("fw", "<u4"), ("started_n", "<u4"),
                      ("round", "<u8"), ("tracked_msg", "<u4"), ("btab_hash", "<u4"), ("G", "<u4"), ("world", "<u4"),
                      ("slot_tab", "<u4", (2 * _abi.MSG_SLOTS,))])
SHARD_HEAD = np.dtype([("lo", "<u4"), ("n", "<u4"), ("m_in", "<u4"), ("in_cur", "<u4"), ("pay_cur", "<u4"),
                       ("pay_rows", "<u4"), ("pad", "<u4", (2,)), ("out_rows", "<u4"), ("pad2", "<u4", (3,))])


class LayoutError(AssertionError):
    """the snapshot is not laid out as this mirror believes"""


class DomainError(ValueError):
    """rows that would leave what the engine guarantees its getters"""


def _sections(head, sh):
    """[(name, dtype, shape)] of one shard, in snap_sections() order"""
    N, n, fw = int(head["n_nodes"]), int(sh["n"]), int(head["fw"])
    pluggable = int(head["manager"]) == _abi.MANAGER_PLUGGABLE
    strategy = int(head["strategy"])
    v = [("flags", "u1", (N,)), ("part", "u1", (N,)), ("hdr", HDR, (n,)),
         ("act", "<u4", (n, _abi.ACTIVE_CAP)), ("pas", "<u4", (n, _abi.PASSIVE_CAP)),
         ("sentm", "<u8", (n, IDMAP_IN)), ("recvm", "<u8", (n, IDMAP_IN)),
         ("mapx", "<u8", (int(sh["pad"][1]), IDMAP_EXT)),
         ("pt_all", "<u4", (n, _abi.PT_MEMBERS_CAP)), ("pt_com", "<u4", (n, _abi.PT_MEMBERS_CAP)),
         ("pt_eag", "<u4", (n, RT_SET)), ("pt_laz", "<u4", (n, RT_SET)), ("pt_rt", "<u4", (n, RT_WORDS)),
         ("pt_out", "<u8", (n, OUT_IN)), ("outx", "<u8", (int(sh["out_rows"]), OUT_EXT)), ("start", "<u4", (n,))]
    if not pluggable:                                   # (a pluggable handle keeps no connection table)
        v.append(("conn", "<u4", (n, _abi.CONN_CAP)))
    v += [("cb", "<u8", (n + 1,)), ("bmask", "<u8", (n,)), ("in_beg", "<u4", (n + 1,)),
          ("inbox", "u1", (int(sh["m_in"]), MSG_BYTES))]
    if pluggable:
        if strategy != _abi.STRATEGY_FULL:
            v.append(("sview", "<u4", (n, _abi.SVIEW_CAP)))
            if strategy == _abi.STRATEGY_SCAMP_V2:
                v.append(("sinv", "<u4", (n, _abi.SVIEW_CAP)))
        else:
            v.append(("fbits", "<u4", (n, 2 * fw)))
        if int(sh["pay_rows"]):
            v.append(("pay", "<u4", (int(sh["pay_rows"]), 2 * fw)))
        if int(sh["pad2"][0]):
            v.append(("pay_imp", "<u4", (int(sh["pad2"][0]), (2 if int(sh["pad"][0]) else 1) * fw)))
    return v


class Shard(dict):
    """name -> view of one shard's sections; .head: its ShardHead"""
    __getattr__ = dict.__getitem__


class Layout:
    def __init__(self, buf, head, started, shards):
        self.buf, self.head, self.started, self.shards = buf, head, started, shards

    def tobytes(self):
        return self.buf.tobytes()


def layout(cfg, snapshot_bytes):
    """the snapshot of one handle (one rank of a world) as named views over a
    writable copy; Layout.tobytes() serialises it again"""
    buf = np.frombuffer(bytearray(snapshot_bytes), np.uint8)
    if buf.size < SNAP_HEAD.itemsize:
        raise LayoutError("shorter than a SnapHead")
    head = buf[: SNAP_HEAD.itemsize].view(SNAP_HEAD)[0]
    want = dict(magic=SNAP_MAGIC, abi=_abi.PSIM_ABI_VERSION, n_nodes=cfg.n_nodes, manager=cfg.manager,
                strategy=cfg.strategy, world=max(int(cfg.shard_world), 1))
    for k, v in want.items():
        if int(head[k]) != int(v):
            raise LayoutError(f"SnapHead.{k} = {int(head[k])}, expected {int(v)}")
    at = SNAP_HEAD.itemsize
    if at + int(head["started_n"]) > buf.size:
        raise LayoutError("the started bytes pass the end")
    started = buf[at: at + int(head["started_n"])]
    at += started.size
    shards = []
    for _ in range(int(head["n_local_shards"])):
        if at + SHARD_HEAD.itemsize > buf.size:
            raise LayoutError("a ShardHead passes the end")
        sh = buf[at: at + SHARD_HEAD.itemsize].view(SHARD_HEAD)[0]
        at += SHARD_HEAD.itemsize
        if int(sh["lo"]) + int(sh["n"]) > cfg.n_nodes or int(sh["pay_cur"]) > 1:
            raise LayoutError(f"ShardHead lo {int(sh['lo'])} n {int(sh['n'])} pay_cur {int(sh['pay_cur'])}")
        s = Shard(head=sh)
        for name, dt, shape in _sections(head, sh):
            nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
            if at + nbytes > buf.size:
                raise LayoutError(f"section {name} of shard lo {int(sh['lo'])} passes the end")
            s[name] = buf[at: at + nbytes].view(dt).reshape(shape)
            at += nbytes
        shards.append(s)
    if at != buf.size:
        raise LayoutError(f"the sections add up to {at} bytes, the snapshot has {buf.size}")
    owned = sorted((int(s.head["lo"]), int(s.head["n"])) for s in shards)
    if any(a[0] + a[1] > b[0] for a, b in zip(owned, owned[1:])):
        raise LayoutError(f"shards overlap: {owned}")
    return Layout(buf, head, started, shards)


# ------------------------------------------------------------- the domain --
HV_FIELDS = ("up", "act", "common", "conn", "slots")
SCAMP_FIELDS = ("up", "view", "in_view")
DIRT = ("self", "dup", "dead")


def _kind(cfg):
    if cfg.manager != _abi.MANAGER_PLUGGABLE:
        return "hv"
    if cfg.strategy == _abi.STRATEGY_SCAMP_V2:
        return "scamp"
    # scamp v1 keeps its view as an OTP set with a slot count in the header
    # (Hdr.pad1[1]) that no plain row determines; full keeps bit rows
    raise DomainError("inject knows HyParView / X-BOT and SCAMP v2 handles only")


def _ids(i, name, ids, cap, n, mask=0):
    """a row of ids: at most `cap` of them, each (its flag bit `mask` dropped) a node id below n"""
    ids = [int(x) for x in ids]
    if len(ids) > cap:
        raise DomainError(f"node {i}: {name} holds {len(ids)} entries, the cap is {cap}")
    for e in ids:
        if not 0 <= e <= NONE or (e & ~mask) >= n:
            raise DomainError(f"node {i}: {name} entry {e:#x} names no node below {n}")
    return ids


def _clean(i, name, ids, up, allow, mask=0):
    """repeated ids, the node's own id and dead targets only where the caller
    says the getter under test defines them"""
    ps = [e & ~mask for e in ids]
    if "dup" not in allow and len(set(ps)) != len(ps):
        raise DomainError(f"node {i}: {name} repeats an id (dirty rows not allowed here)")
    if "self" not in allow and i in ps:
        raise DomainError(f"node {i}: {name} holds the node itself (dirty rows not allowed here)")
    if "dead" not in allow and any(not up[p] for p in ps):
        raise DomainError(f"node {i}: {name} names a dead node (dirty rows not allowed here)")


def validate(cfg, rows, allow=()):
    """rows: one dict per node id.  Returns them normalised (every field of
    the handle's kind present); raises DomainError, touching no device."""
    n = int(cfg.n_nodes)
    kind = _kind(cfg)
    fields = HV_FIELDS if kind == "hv" else SCAMP_FIELDS
    if set(allow) - set(DIRT):
        raise DomainError(f"unknown kind of dirt: {sorted(set(allow) - set(DIRT))}")
    if len(rows) != n:
        raise DomainError(f"{len(rows)} rows for {n} nodes")
    for i, r in enumerate(rows):
        unknown = set(r) - set(fields)
        if unknown:
            raise DomainError(f"node {i}: unknown field(s) {sorted(unknown)} for a {kind} handle")
    up = [bool(r.get("up", True)) for r in rows]
    out = []
    for i, r in enumerate(rows):
        o = dict(up=up[i])
        if kind == "hv":
            # act: k_hist_out and k_pack_act run to act_n over an ACTIVE_CAP row and
            # k_hist_out reads flags[p] of every entry unguarded: count <= cap, id < n.
            # (k_gm_filter, k_hist_sym, k_cc_hook, k_tm_rows and k_rl_* test p < n themselves.)
            o["act"] = _ids(i, "act", r.get("act", ()), _abi.ACTIVE_CAP, n)
            _clean(i, "act", o["act"], up, allow)
            # common: k_tm_rows and k_rl_* clamp com_n to the row and test the masked id
            # against N before flags[]; an entry is an id or id | MAP_BIT
            o["common"] = _ids(i, "common", r.get("common", ()), _abi.PT_MEMBERS_CAP, n, MAP_BIT)
            # conn: read by k_rl_* only, compared against p and p | CONN_DOWN, never
            # used as an index; CONN_CLOSING entries are X-BOT's and no getter defines them
            o["conn"] = _ids(i, "conn", r.get("conn", ()), _abi.CONN_CAP, n, CONN_DOWN)
            # slots: k_tm_rows reads the counts as bytes, clamps each run to the 64-entry
            # pool and tests masked ids against N; the engine never lets the runs of a
            # pool pass 64 entries in all nor gives two slots one root
            slots = list(r.get("slots", ()))
            if len(slots) > _abi.PT_ROOTS:
                raise DomainError(f"node {i}: {len(slots)} root slots, the cap is {_abi.PT_ROOTS}")
            o["slots"] = []
            for root, eag, laz in slots:
                root = int(root)
                if root != NONE and (not root & MAP_BIT or (root & ~MAP_BIT) >= n):
                    raise DomainError(f"node {i}: slot root {root:#x} is no id | MAP_BIT below {n}")
                o["slots"].append((root, _ids(i, "eager", eag, RT_SET, n, MAP_BIT),
                                   _ids(i, "lazy", laz, RT_SET, n, MAP_BIT)))
            taken = [s[0] for s in o["slots"] if s[0] != NONE]
            if len(set(taken)) != len(taken):
                raise DomainError(f"node {i}: two slots of one root")
            for k, what in ((1, "eager"), (2, "lazy")):
                if sum(len(s[k]) for s in o["slots"]) > RT_SET:
                    raise DomainError(f"node {i}: the {what} pool holds more than {RT_SET} entries")
        else:
            # view / in_view: k_sh_rows and k_sh_inv clamp the lengths to SVIEW_CAP and test
            # id < N before flags[] (sh_live); the CSR they build holds live ids only, which
            # is what k_gm_push / k_lt_push index seen[] and dist[] with
            o["view"] = _ids(i, "view", r.get("view", ()), _abi.SVIEW_CAP, n)
            _clean(i, "view", o["view"], up, allow)
            o["in_view"] = _ids(i, "in_view", r.get("in_view", ()), _abi.SVIEW_CAP, n)
        out.append(o)
    return out


# -------------------------------------------------------------- injection --
def _write(lay, rows, kind):
    for s in lay.shards:
        lo, n = int(s.head["lo"]), int(s.head["n"])
        # the flags are replicated: every shard and rank holds all N
        fl = s.flags
        fl[:] = (fl & ~np.uint8(F_UP)) | np.array([r["up"] for r in rows], np.uint8)
        hdr = s.hdr
        for li in range(n):
            r = rows[lo + li]
            if kind == "scamp":
                hdr["act_n"][li], hdr["pas_n"][li] = len(r["view"]), len(r["in_view"])
                s.sview[li] = 0
                s.sview[li, : len(r["view"])] = r["view"]
                s.sinv[li] = 0
                s.sinv[li, : len(r["in_view"])] = r["in_view"]
                continue
            hdr["act_n"][li], hdr["pas_n"][li] = len(r["act"]), 0
            hdr["all_n"][li] = hdr["com_n"][li] = len(r["common"])
            hdr["conn_n"][li] = len(r["conn"])
            hdr["conn_dn"][li] = sum(1 for e in r["conn"] if e & CONN_DOWN)
            for name, key in (("act", "act"), ("pt_all", "common"), ("pt_com", "common"), ("conn", "conn")):
                s[name][li] = 0
                s[name][li, : len(r[key])] = r[key]
            s.pas[li] = 0
            rt = np.zeros(RT_WORDS, np.uint32)
            rt[: _abi.PT_ROOTS] = NONE
            eag = [e for sl in r["slots"] for e in sl[1]]
            laz = [e for sl in r["slots"] for e in sl[2]]
            for k, (root, e, z) in enumerate(r["slots"]):
                rt[k] = root
                rt[_abi.PT_ROOTS] |= len(e) << (8 * k)
                rt[_abi.PT_ROOTS + 1] |= len(z) << (8 * k)
            s.pt_rt[li] = rt
            s.pt_eag[li] = 0
            s.pt_eag[li, : len(eag)] = eag
            s.pt_laz[li] = 0
            s.pt_laz[li, : len(laz)] = laz


def _read_back(sim, rows, kind):
    if kind == "scamp":
        v = sim.strategy_nodes()
        for i, r in enumerate(rows):
            assert bool(v["up"][i]) == r["up"], f"node {i}: up"
            assert [int(x) for x in v["view"][i][: int(v["view_n"][i])]] == r["view"], f"node {i}: view"
            assert [int(x) for x in v["in_view"][i][: int(v["in_n"][i])]] == r["in_view"], f"node {i}: in_view"
        return
    v = sim.nodes()
    for i, r in enumerate(rows):
        assert bool(v["up"][i]) == r["up"], f"node {i}: up"
        assert [int(x) for x in v["act"][i][: int(v["act_n"][i])]] == r["act"], f"node {i}: act"
        assert int(v["pas_n"][i]) == 0, f"node {i}: pas_n"
        assert [int(x) for x in v["pt_common"][i][: int(v["pt_common_n"][i])]] == r["common"], f"node {i}: common"
        assert [int(x) for x in v["conn"][i][: int(v["conn_n"][i])]] == r["conn"], f"node {i}: conn"
        en, ln = [int(x) for x in v["pt_eager_n"][i]], [int(x) for x in v["pt_lazy_n"][i]]
        slots = r["slots"] + [(NONE, [], [])] * (_abi.PT_ROOTS - len(r["slots"]))
        for k, (root, e, z) in enumerate(slots):
            eo, zo = sum(en[:k]), sum(ln[:k])
            assert int(v["pt_root"][i][k]) == root, f"node {i}: root of slot {k}"
            assert [int(x) for x in v["pt_eager"][i][eo: eo + en[k]]] == e, f"node {i}: eager run {k}"
            assert [int(x) for x in v["pt_lazy"][i][zo: zo + ln[k]]] == z, f"node {i}: lazy run {k}"


def inject(sim, rows, allow=()):
    """put `rows` (one dict per node: up, act, common, conn, slots on a
    HyParView / X-BOT handle; up, view, in_view on a SCAMP v2 handle; a field
    left out is empty, up is True) into `sim`, a Simulator or LoopbackRanks
    whose every id has joined and that has stepped a round.  allow: the kinds
    of dirt ("self", "dup", "dead") the getters about to be called define for
    the link rows.  Returns the normalised rows."""
    cfg = sim.cfg
    rows = validate(cfg, rows, allow)           # (raises before any device call)
    kind = _kind(cfg)
    ranked = hasattr(sim, "ranks")
    snaps = sim.snapshot() if ranked else [sim.snapshot()]
    cfgs = [s.cfg for s in sim.ranks] if ranked else [cfg]
    lays = [layout(c, b) for c, b in zip(cfgs, snaps)]
    owned = sorted(x for lay in lays for s in lay.shards for x in range(int(s.head["lo"]), int(s.head["lo"]) + int(s.head["n"])))
    if owned != list(range(int(cfg.n_nodes))):
        raise LayoutError("the shards of the snapshot(s) do not own every id exactly once")
    for lay in lays:
        _write(lay, rows, kind)
    data = [lay.tobytes() for lay in lays]
    sim.restore(data if ranked else data[0])
    _read_back(sim, rows, kind)
    return rows
