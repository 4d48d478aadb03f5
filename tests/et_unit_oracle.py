"""TEST INFRASTRUCTURE ONLY -- plain torch statements of the Equivariant Transformer's edge sweeps (csrc/tn_et.hip,
csrc/tn_et_g16.hip; reference torchmd_et.py:376-426 and its adjoint) in the kernels' layouts, dtype-generic: the unit tests
evaluate them in float64 (tests/test_gpu_et_unit.py) and, for the rounding floor, in float32 (tools/et_unit_floor.py).
tests/test_et_unit_oracle.py keeps every hand-written adjoint honest against autograd of the forward statement.

Graph: the engine's symmetric CSR as a dict (tests/et_unit_cases.py): rows / col / epair / esign per entry e = (i <- j), i = rows[e]
the message TARGET, j = col[e] its source, p = epair[e] (P on the self edge), esign +1 where i is the pair's first atom (j < i).
rhat(i <- j) = -esign prhat[p], 0 on the self edge.  Layout `lay` = dict(F, hd, dk_off, dv_off, vc): dkv / tkv [P + 1, Wd] hold the
key projection's F columns at dk_off and the value projection's 3 F at dv_off (-1: no such projection: factor 1, tangent 0).
"""
import torch


def silu(x):
    return x * torch.sigmoid(x)


def dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def _heads(t, hd):
    """[E, F] -> [E, H]: sum over the channels of each head"""
    return t.reshape(t.shape[0], -1, hd).sum(-1)


def _chan(t, hd):
    """[E, H] -> [E, F]: a head's value on each of its channels"""
    return t.repeat_interleave(hd, dim=1)


def edge_terms(g, d, lay, delta=None, rhat_c=None):
    """Every per-edge quantity of the forward sweep.  delta [E, F] (optional) moves the pair's distance per (edge, channel):
    dkv + tkv delta and C + dC delta (the attention cutoff of a head moves with its FIRST channel's delta, as the kernels book
    it); rhat_c [E, 3, F] (optional) replaces rhat per channel.  Both exist so that autograd can state the slot sums."""
    F, hd, vc = lay["F"], lay["hd"], lay["vc"]
    i, j, p, sg = g["rows"], g["col"], g["epair"], g["esign"].to(d["qkv"].dtype)
    dt, dev = d["qkv"].dtype, d["qkv"].device
    E = i.numel()
    one = torch.ones(E, F, dtype=dt, device=dev)
    q, k, vx, v1, v2 = (d["qkv"][:, n * F:(n + 1) * F] for n in range(5))

    def rows_of(off):
        if off < 0:
            return one
        r = d["dkv"][p, off:off + F]
        return r if delta is None else r + d["tkv"][p, off:off + F] * delta

    dko, dvo = lay["dk_off"], lay["dv_off"]
    dk, dvx = rows_of(dko), rows_of(dvo)
    dv1, dv2 = rows_of(dvo + F if dvo >= 0 else -1), rows_of(dvo + 2 * F if dvo >= 0 else -1)
    C = d["C"][p][:, None].expand(E, F)
    if delta is not None:
        C = C + d["dC"][p][:, None] * delta
    cv = C if vc else one
    ca = one[:, ::hd] if vc else C[:, ::hd]  # [E, H]
    a = _heads(q[i] * k[j] * dk, hd)
    A = silu(a) * ca
    sx, s1, s2 = vx[j] * cv * dvx, v1[j] * cv * dv1, v2[j] * cv * dv2
    prhat = torch.cat([d["prhat"], torch.zeros(1, 3, dtype=dt, device=dev)])
    rhat = -sg[:, None] * prhat[p]  # [E, 3]; 0 on the self edge
    rh = rhat[:, :, None].expand(E, 3, F) if rhat_c is None else rhat_c
    return dict(i=i, j=j, p=p, sg=sg, q=q, k=k, vx=vx, v1=v1, v2=v2, dk=dk, dvx=dvx, dv1=dv1, dv2=dv2, cv=cv, ca=ca, a=a, A=A, sx=sx,
                s1=s1, s2=s2, rhat=rhat, rh=rh)


def attn_forward(g, d, lay, delta=None, rhat_c=None):
    """-> (xagg [N, F], vagg [N, 3, F]):  xagg[i] = sum_e sx A,  vagg[i, x] = sum_e vec[j, x] s1 + s2 rhat_x"""
    t = edge_terms(g, d, lay, delta, rhat_c)
    N, F = d["qkv"].shape[0], lay["F"]
    xagg = torch.zeros(N, F, dtype=t["sx"].dtype, device=t["sx"].device).index_add(0, t["i"], t["sx"] * _chan(t["A"], lay["hd"]))
    vm = d["vec"][t["j"]] * t["s1"][:, None, :] + t["s2"][:, None, :] * t["rh"]
    vagg = torch.zeros(N, 3, F, dtype=vm.dtype, device=vm.device).index_add(0, t["i"], vm)
    return xagg, vagg


def attn_adjoint(g, d, lay):
    """The hand-written adjoint of sum(g_xagg xagg) + sum(g_vagg vagg), per directed edge in both roles of its atoms.
    -> dict(g_qkv [N, 5 F], g_vec [N, 3, F] (what the sweep ADDS), gd_c / gd_abs [E, F], gr_c / gr_abs [E, 3, F]): per channel, the
    edge's d / d d(pair) and d / d rhat(i <- j), and the sums of the absolute values of their terms."""
    F, hd, vc = lay["F"], lay["hd"], lay["vc"]
    t = edge_terms(g, d, lay)
    i, j, p = t["i"], t["j"], t["p"]
    N = d["qkv"].shape[0]
    dt, dev = d["qkv"].dtype, d["qkv"].device
    gx, gv = d["g_xagg"][i], d["g_vagg"][i]  # of the TARGET
    zero = torch.zeros(i.numel(), F, dtype=dt, device=dev)

    def tang(off):
        return zero if off < 0 else d["tkv"][p, off:off + F]

    dko, dvo = lay["dk_off"], lay["dv_off"]
    tk, tvx = tang(dko), tang(dvo)
    tv1, tv2 = tang(dvo + F if dvo >= 0 else -1), tang(dvo + 2 * F if dvo >= 0 else -1)
    Ac = _chan(t["A"], hd)
    # ---- role TARGET of the row atom i: message j -> i
    g_sx = gx * Ac
    g_A = _heads(gx * t["sx"], hd)
    g_s1 = (gv * d["vec"][j]).sum(1)
    g_s2 = (gv * t["rhat"][:, :, None]).sum(1)
    g_a = g_A * dsilu(t["a"]) * t["ca"]
    g_ac = _chan(g_a, hd)
    cv = t["cv"]
    # the same sums with every elementary product replaced by its absolute value: the scale of the channel's terms (g_A, g_s1 and
    # g_s2 are sums themselves, over the head's channels and the three components)
    A_abs = _heads((gx * t["sx"]).abs(), hd)
    s1_abs = (gv * d["vec"][j]).abs().sum(1)
    s2_abs = (gv * t["rhat"][:, :, None]).abs().sum(1)
    ac_abs = _chan(A_abs * dsilu(t["a"]).abs() * t["ca"], hd)
    terms = [cv * g_sx * t["vx"][j] * tvx, cv * g_s1 * t["v1"][j] * tv1, cv * g_s2 * t["v2"][j] * tv2, g_ac * t["q"][i] * t["k"][j] * tk]
    sizes = [terms[0].abs(), (cv * s1_abs * t["v1"][j] * tv1).abs(), (cv * s2_abs * t["v2"][j] * tv2).abs(), (ac_abs * t["q"][i] * t["k"][j] * tk).abs()]
    dC = d["dC"][p][:, None]
    if vc:
        terms += [g_sx * t["vx"][j] * t["dvx"] * dC, g_s1 * t["v1"][j] * t["dv1"] * dC, g_s2 * t["v2"][j] * t["dv2"] * dC]
        sizes += [terms[4].abs(), (s1_abs * t["v1"][j] * t["dv1"] * dC).abs(), (s2_abs * t["v2"][j] * t["dv2"] * dC).abs()]
    else:  # the attention cutoff of a head, booked on the head's first channel
        first = torch.zeros(F, dtype=dt, device=dev)
        first[::hd] = 1
        terms += [_chan(g_A * silu(t["a"]), hd) * first * dC]
        sizes += [(_chan(A_abs * silu(t["a"]), hd) * first * dC).abs()]
    gd_c, gd_abs = sum(terms), sum(sizes)
    gr_c = gv * t["s2"][:, None, :]
    z = lambda *s: torch.zeros(*s, dtype=dt, device=dev)
    g_q = z(N, F).index_add(0, i, g_ac * t["k"][j] * t["dk"])
    # ---- role SOURCE of the atom j: the same message seen from its sender
    g_k = z(N, F).index_add(0, j, g_ac * t["q"][i] * t["dk"])
    g_vx = z(N, F).index_add(0, j, g_sx * cv * t["dvx"])
    g_v1 = z(N, F).index_add(0, j, g_s1 * cv * t["dv1"])
    g_v2 = z(N, F).index_add(0, j, g_s2 * cv * t["dv2"])
    g_vec = z(N, 3, F).index_add(0, j, gv * t["s1"][:, None, :])
    return dict(g_qkv=torch.cat([g_q, g_k, g_vx, g_v1, g_v2], 1), g_vec=g_vec, gd_c=gd_c, gd_abs=gd_abs, gr_c=gr_c, gr_abs=gr_c.abs(),
                g_a=g_a, g_sx=g_sx, g_s1=g_s1, g_s2=g_s2, t=t)


def slot_index(g):
    """slot 2 p + dir of every entry (dir 0: esign > 0, 1: esign < 0); -1 for the self edge, which owns no slot"""
    s = 2 * g["epair"] + (g["esign"] < 0).long()
    return torch.where(g["esign"] == 0, torch.full_like(s, -1), s)


def slot_sums(g, adj, lay, group):
    """The slot arrays of the reverse sweep: one per `group` channels (32: tile kernels, 64: row kernels).
    -> (gd2 [W, 2 P], gd_scale, gr2 [W, 2 P, 3], gr_scale): partial sums over the array's channels and the sums of the absolute
    values of their terms."""
    F, P = lay["F"], g["P"]
    W = -(-F // group)
    sl = slot_index(g)
    own = sl >= 0
    idx = sl[own]

    def fold(c):  # [E, (3,) F] -> [W, 2 P (, 3)]
        c = c[own]
        pad = W * group - F
        if pad:
            c = torch.cat([c, torch.zeros(*c.shape[:-1], pad, dtype=c.dtype, device=c.device)], -1)
        part = c.reshape(*c.shape[:-1], W, group).sum(-1)  # [Eo, (3,) W]
        out = torch.zeros(2 * P, *part.shape[1:], dtype=c.dtype, device=c.device).index_add(0, idx, part)
        return out.movedim(-1, 0)  # [W, 2 P (, 3)]

    return fold(adj["gd_c"]), fold(adj["gd_abs"]), fold(adj["gr_c"]), fold(adj["gr_abs"])


def pair_combine(gd2, gr2, gd_extra, P):
    """gd[p] = gd_extra[2 p] + sum_w gd2[w, 2 p] + gd2[w, 2 p + 1];  g_rhat[p] = sum_w -gr2[w, 2 p] + gr2[w, 2 p + 1]
    -> (gd, gd_scale, g_rhat, g_rhat_scale)"""
    a, b = gd2[:, 0:2 * P:2], gd2[:, 1:2 * P:2]
    ra, rb = gr2[:, 0:2 * P:2], gr2[:, 1:2 * P:2]
    e = gd_extra[0:2 * P:2]
    return (e + (a + b).sum(0), e.abs() + (a.abs() + b.abs()).sum(0), (rb - ra).sum(0), (rb.abs() + ra.abs()).sum(0))


def nbr_embed(g, z, emb, embN_atoms, Wn):
    """xcat [N, 2 F] = emb[z_i] | sum_{j != i} Wn[p] embN[z_j]   (embN_atoms [N, F] = embN[z])"""
    i, j, p = g["rows"], g["col"], g["epair"]
    m = (i != j).to(Wn.dtype)[:, None]
    nbr = torch.zeros_like(embN_atoms).index_add(0, i, Wn[p] * embN_atoms[j] * m)
    return torch.cat([emb[z], nbr], 1)


def nbr_embed_bwd(g, embN_atoms, g_nbr, dWn):
    """what is ADDED to gd2[2 p]: sum_c (g_nbr[i] embN[z_j] + g_nbr[j] embN[z_i]) dWn[p], i = pair_i[p], j = pair_j[p]
    -> (value [P], scale [P])"""
    i, j, P = g["pair_i"], g["pair_j"], g["P"]
    t1, t2 = g_nbr[i] * embN_atoms[j] * dWn[:P], g_nbr[j] * embN_atoms[i] * dWn[:P]
    return (t1 + t2).sum(1), (t1.abs() + t2.abs()).sum(1)


def train_nbr(g, embN_atoms, Wn, g_nbr):
    """-> (slots [2, P, F]: slots[dir, p] = g_nbr[i] embN[z_j] of the entry (i <- j);  gEN [N, F] = sum_{j != i} g_nbr[j] Wn[p])"""
    i, j, p, P = g["rows"], g["col"], g["epair"], g["P"]
    ns = i != j
    F = Wn.shape[1]
    slots = torch.zeros(2 * P, F, dtype=Wn.dtype, device=Wn.device)
    slots[slot_index(g)[ns]] = (g_nbr[i] * embN_atoms[j])[ns]
    gEN = torch.zeros_like(embN_atoms).index_add(0, i[ns], (g_nbr[j] * Wn[p])[ns])
    return slots.reshape(P, 2, F).transpose(0, 1), gEN


def train_filter(g, d, lay):
    """The adjoint of the filter rows dkv per directed edge (the TARGET role): -> (slots [2, P, Wd], self_rows [N, Wd]); columns the
    layout does not use are NaN (the kernel does not write them)."""
    F, Wd, P = lay["F"], d["dkv"].shape[1], g["P"]
    adj = attn_adjoint(g, d, lay)
    t = adj["t"]
    i, j = t["i"], t["j"]
    rows = torch.full((i.numel(), Wd), float("nan"), dtype=d["qkv"].dtype, device=d["qkv"].device)
    if lay["dk_off"] >= 0:
        rows[:, lay["dk_off"]:lay["dk_off"] + F] = _chan(adj["g_a"], lay["hd"]) * t["q"][i] * t["k"][j]
    if lay["dv_off"] >= 0:
        o = lay["dv_off"]
        rows[:, o:o + F] = t["cv"] * adj["g_sx"] * t["vx"][j]
        rows[:, o + F:o + 2 * F] = t["cv"] * adj["g_s1"] * t["v1"][j]
        rows[:, o + 2 * F:o + 3 * F] = t["cv"] * adj["g_s2"] * t["v2"][j]
    sl = slot_index(g)
    own = sl >= 0
    slots = torch.zeros(2 * P, Wd, dtype=rows.dtype, device=rows.device)
    slots[sl[own]] = rows[own]
    self_rows = torch.zeros(d["qkv"].shape[0], Wd, dtype=rows.dtype, device=rows.device)
    self_rows[i[~own]] = rows[~own]
    return slots.reshape(P, 2, Wd).transpose(0, 1), self_rows


def train_gpre(slots, self_sum, pre):
    """g_pre [P + 1, Wd] = (slots[0] + slots[1]) silu'(pre) for the pairs, self_sum silu'(pre[P]) for the self pair"""
    return torch.cat([slots[0] + slots[1], self_sum[None, :]]) * dsilu(pre)


def per_row_rel_err(got, ref):
    """max over rows (atoms, pairs) of max|got - ref| / max|ref|, each row's block normalised by its own maximum; positions where
    the reference is NaN (not written by the kernel) are left out"""
    n = ref.shape[0]
    if n == 0:
        return 0.0
    r = ref.reshape(n, -1).double()
    keep = ~torch.isnan(r)
    dlt = torch.where(keep, (got.reshape(n, -1).double() - r).abs(), torch.zeros_like(r)).amax(1)
    s = torch.where(keep, r.abs(), torch.zeros_like(r)).amax(1).clamp_min(1e-300)
    return float((dlt / s).max())


def scaled_err(got, ref, scale):
    """max |got - ref| / scale, elementwise: scale = the sum of the absolute values of the element's terms"""
    if ref.numel() == 0:
        return 0.0
    return float(((got.double() - ref.double()).abs() / scale.double().clamp_min(1e-300)).max())
