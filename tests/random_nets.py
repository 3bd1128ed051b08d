"""Seeded random CNN graphs in planer's IR (shared by the GPU fuzz tests and the CPU plan-compiler tests)."""
import numpy as np

from planer_amd.irgen.builder import GraphBuilder


def random_net(seed):
    r = np.random.default_rng(seed)
    gb = GraphBuilder(["x"])
    n, c0, h0 = int(r.choice([1, 2, 3])), int(r.choice([1, 3, 4, 8])), int(r.choice([8, 12, 16, 20]))
    live = {"x": (c0, h0, h0)}
    uid = [0]

    def new(prefix):
        uid[0] += 1
        return "%s%d" % (prefix, uid[0])

    def pick(pred=lambda s: True):
        names = [k for k, s in live.items() if pred(s)]
        return names[int(r.integers(len(names)))] if names else None

    for _ in range(int(r.integers(4, 12))):
        kind = r.choice(["conv", "conv", "conv", "conv", "pool", "up", "concat", "add", "sigmoid", "relu"])
        src = pick()
        c, h, w = live[src]
        if kind == "conv":
            k = int(r.choice([1, 3, 3, 5])); st = int(r.choice([1, 1, 2])); co = int(r.choice([3, 4, 8, 12, 16, 20, 32]))
            if h < 3 and st == 2:
                st = 1
            K = gb.init(new("K"), (r.standard_normal((co, c, k, k)) * np.sqrt(2.0 / (c * k * k))).astype(np.float32))
            ins = [src, K]
            if r.random() < 0.5:
                ins.append(gb.init(new("B"), (r.standard_normal(co) * 0.1).astype(np.float32)))
            ho = (h + 2 * (k // 2) - k + st) // st
            cur = gb.op("conv", ins, new("c"), group=1, strides=[st, st], dilations=[1, 1], pads=[k // 2] * 4)
            shape = (co, ho, ho)
            if r.random() < 0.7:
                sc = gb.init(new("s"), r.uniform(0.5, 1.5, (1, co, 1, 1)).astype(np.float32))
                sh = gb.init(new("t"), (r.standard_normal((1, co, 1, 1)) * 0.1).astype(np.float32))
                cur = gb.op("batchnorm", [cur, sc, sh], new("b"))
            other = pick(lambda s: s == shape)
            if other is not None and r.random() < 0.5:
                cur = gb.op("add", [cur, other], new("a"))
            act = r.choice(["relu", "leakyrelu", "none"])
            if act == "relu":
                cur = gb.op("relu", cur, new("r"))
            elif act == "leakyrelu":
                cur = gb.op("leakyrelu", cur, new("l"), alpha=0.1)
            live[cur] = shape
        elif kind == "pool" and h >= 4:
            k, st, pd = [(2, 2, 0), (3, 2, 1)][int(r.integers(2))]
            op = "maxpool" if r.random() < 0.7 else "averagepool"
            ho = (h + 2 * pd - k + st) // st
            live[gb.op(op, src, new("p"), w=[k, k], pads=[pd] * 4, strides=[st, st])] = (c, ho, ho)
        elif kind == "up" and h <= 16:
            f = gb.init(new("f"), np.array([1, 1, 2, 2], np.float32))
            live[gb.op("upsample", [src, f], new("u"), mode="nearest")] = (c, 2 * h, 2 * w)
        elif kind == "concat":
            other = pick(lambda s: s[1:] == (h, w))
            live[gb.op("concat", [src, other], new("k"), axis=1)] = (c + live[other][0], h, w)
        elif kind == "add":
            other = pick(lambda s: s == (c, h, w))
            live[gb.op("add", [src, other], new("a"))] = (c, h, w)
        elif kind == "sigmoid":
            live[gb.op("sigmoid", src, new("g"))] = (c, h, w)
        elif kind == "relu" and src != "x":
            live[gb.op("relu", src, new("r"))] = (c, h, w)     # in place in the reference: later readers of `src` see it
    names = [k for k in live if k != "x"] or ["x"]
    outs = [names[-1]]
    if len(names) > 2 and r.random() < 0.5:
        outs.append(names[int(r.integers(len(names) - 1))])
    if r.random() < 0.7:
        src = names[int(r.integers(len(names)))]
        c = live[src][0]
        gp = gb.op("gap", src, new("q"))
        fl = gb.op("flatten", gp, new("v"))
        W = gb.init(new("W"), (r.standard_normal((10, c)) * 0.2).astype(np.float32))
        Bd = gb.init(new("D"), r.standard_normal(10).astype(np.float32))
        outs.append(gb.op("dense", [fl, W, Bd], new("y"), shp=[c, 10]))
    g, blob = gb.finish(outs)
    xs = [r.standard_normal((n, c0, h0, h0)).astype(np.float32) for _ in range(2)]
    return g, blob, xs


def random_net_real(seed):
    """Seeded CNNs at real layer sizes, for the plan audit (tests/plan_audit.py): channels 16 .. 256 plus some C % 4 != 0, maps
    of 7 .. 56 pixels, batch 1 .. 4 (8 where a 21-pixel map can give the mixed-tile Winograd its 64 GEMM columns).  Blocks:
    runs of 3x3 stride-1 convs whose tensors have second readers and in-place readers (Winograd chains, keep_y), stride-2 forks
    with a 1x1 stride-2 projection (conv pairs), Darknet 1x1 -> 3x3 pairs (conv1x1_wino_in), inverted residuals with a
    depthwise conv, grouped and dilated convs, ConvTranspose and nearest-upsample steps into a concat, BN / residual / ReLU /
    leaky / clip tails, and a head with a partial channel quad.  The input has per-channel magnitudes 2^U(-3, 3) and a DC
    offset, as ref64.skewed_operands draws them.  -> (graph, blob, [x])"""
    r = np.random.default_rng(seed)
    gb = GraphBuilder(["x"])
    h0 = int(r.choice([14, 21, 21, 28, 42, 42, 56, 30]))
    n = 8 if h0 in (21, 42) and r.random() < 0.6 else int(r.choice([1, 2, 3, 4]))
    c0 = int(r.choice([3, 3, 16]))
    live = {"x": (c0, h0)}
    skips = {}
    uid = [0]

    def new(prefix):
        uid[0] += 1
        return "%s%d" % (prefix, uid[0])

    def conv(src, cout, k=3, s=1, d=1, g=1, act=None, res=None, bias=None, bn=True):
        cin, h = live[src]
        std = np.sqrt(2.0 / (cin // g * k * k))
        K = gb.init(new("K"), (r.standard_normal((cout, cin // g, k, k)) * std).astype(np.float32))
        ins = [src, K]
        if bias if bias is not None else r.random() < 0.3:
            ins.append(gb.init(new("B"), (r.standard_normal(cout) * 0.1).astype(np.float32)))
        p = d * (k // 2)
        cur = gb.op("conv", ins, new("c"), group=g, strides=[s, s], dilations=[d, d], pads=[p] * 4)
        ho = (h + 2 * p - d * (k - 1) - 1) // s + 1
        if bn:
            sc = gb.init(new("s"), r.uniform(0.5, 1.5, (1, cout, 1, 1)).astype(np.float32))
            sh = gb.init(new("t"), (r.standard_normal((1, cout, 1, 1)) * 0.1).astype(np.float32))
            cur = gb.op("batchnorm", [cur, sc, sh], new("b"))
        act = act or str(r.choice(["relu", "relu", "leaky", "clip", "none"]))
        post = res is not None and act == "leaky" and r.random() < 0.5       # Darknet: residual after the activation
        if res is not None and not post:
            cur = gb.op("add", [cur, res], new("a"))
        if act == "relu":
            cur = gb.op("relu", cur, new("r"))
        elif act == "leaky":
            cur = gb.op("leakyrelu", cur, new("l"), alpha=0.1)
        elif act == "clip":
            cur = gb.op("clip", cur, new("k"), min=0.0, max=6.0)
        if post:
            cur = gb.op("add", [cur, res], new("a"))
        live[cur] = (cout, ho)
        return cur

    def wide(c):
        return int(min(256, max(16, c)))

    cur = conv("x", int(r.choice([16, 32, 64])), act="relu", bias=False)
    for _ in range(int(r.integers(4, 9))):
        c, h = live[cur]
        kind = str(r.choice(["chain", "chain", "fork", "darknet", "dw", "grouped", "dilated", "up", "odd"]))
        if 2 * h in skips and r.random() < 0.5:
            kind = "up"
        if kind == "fork" and h >= 8:
            skips[h] = cur
            co = wide(2 * c if r.random() < 0.7 else c)
            a = conv(cur, co, s=2, act="relu")
            b = conv(a, co, act="none")
            p = conv(cur, co, k=1, s=2, act="none")                  # the projection, in ResNet's order
            cur = gb.op("relu", gb.op("add", [b, p], new("a")), new("r"))
            live[cur] = live[b]
        elif kind == "chain":
            co = int(r.choice([16, 32, 64, 128, 256])) if c % 4 else c
            y = conv(cur, co) if co != c else cur
            first = y
            ys = [y]
            for i in range(int(r.integers(2, 4))):
                res = first if i > 0 and r.random() < 0.5 else None     # a second reader of the run's start: kept tensor
                y = conv(y, co, res=res)
                ys.append(y)
            if r.random() < 0.5 and len(ys) > 2:
                z = gb.op("relu", ys[1], new("r"))                      # an in-place reader of a tensor inside the run
                live[z] = live[ys[1]]
                y = gb.op("add", [y, z], new("a"))
                live[y] = live[ys[-1]]
            cur = y
        elif kind == "darknet" and c >= 16 and c % 8 == 0:
            y1 = conv(cur, c // 2, k=1, act="leaky")
            cur = conv(y1, c, act="leaky", res=cur)
        elif kind == "dw":
            e = wide(int(c * r.choice([2, 4])))
            y = conv(cur, e, k=1, act="clip")
            s = int(r.choice([1, 2])) if h >= 8 else 1
            y = conv(y, e, s=s, g=e, act="clip")
            co = c if s == 1 and r.random() < 0.6 else wide(int(r.choice([16, 24, 32, 64])))
            cur = conv(y, co, k=1, act="none", res=cur if co == c and s == 1 else None)
        elif kind == "grouped" and c % 8 == 0:
            g = int(r.choice([2, 4]))
            cur = conv(cur, c, g=g, d=int(r.choice([1, 2])))
        elif kind == "dilated":
            cur = conv(cur, c, d=2)
        elif kind == "up" and 2 * h in skips:
            skip = skips.pop(2 * h)
            cs = live[skip][0]
            if r.random() < 0.7:
                k = int(r.choice([2, 3]))
                co = wide(int(r.choice([c // 2, c // 4, 20])))
                Kt = gb.init(new("T"), (r.standard_normal((c, co, k, k)) * np.sqrt(4.0 / (c * k * k))).astype(np.float32))
                ins = [cur, Kt] + ([gb.init(new("B"), (r.standard_normal(co) * 0.1).astype(np.float32))] if k == 2 else [])
                p, op = (0, 0) if k == 2 else (1, 1)
                u = gb.op("convtranspose", ins, new("u"), strides=[2, 2], dilations=[1, 1], pads=[p] * 4,
                          output_padding=[op, op], group=1)
                live[u] = (co, 2 * h)
                if k == 3:
                    u = gb.op("relu", u, new("r"))
                    live[u] = (co, 2 * h)
            else:
                f = gb.init(new("f"), np.array([1, 1, 2, 2], np.float32))
                u = gb.op("upsample", [cur, f], new("u"), mode="nearest")
                live[u] = (c, 2 * h)
            cur = gb.op("concat", [u, skip], new("k"), axis=1)
            live[cur] = (live[u][0] + cs, 2 * h)
        elif kind == "odd":
            cur = conv(cur, int(r.choice([6, 10, 18, 30])), k=int(r.choice([1, 3])))
        else:
            cur = conv(cur, c, act="relu")
    outs = [cur]
    c, h = live[cur]
    outs.append(conv(cur, int(r.choice([6, 18, 255 if c <= 64 else 30])), k=1, act="none", bias=True, bn=False))
    if r.random() < 0.5:
        gp = gb.op("gap", cur, new("q"))
        fl = gb.op("flatten", gp, new("v"))
        W = gb.init(new("W"), (r.standard_normal((10, c)) * 0.2).astype(np.float32))
        Bd = gb.init(new("D"), r.standard_normal(10).astype(np.float32))
        outs.append(gb.op("dense", [fl, W, Bd], new("y"), shp=[c, 10]))
    g, blob = gb.finish(outs)
    x = r.standard_normal((n, c0, h0, h0)) * 2.0 ** r.uniform(-3, 3, (1, c0, 1, 1)) + float(r.choice([0.0, 4.0]))
    return g, blob, [x.astype(np.float32)]
