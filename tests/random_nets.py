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


Q4OPS_BLOCKS = ("instnorm", "pad", "groupnorm", "shuffle", "unshuffle", "linear", "dilated")


def random_net_q4ops(seed):
    """Seeded small CNNs made of the steps the channel-quad plans gained after the conv kernels, for the plan audit
    (tests/plan_audit.py): maps of 10 .. 40 pixels (H != W, sides that 2 and 4 do not divide among them), channels 4 .. 64 with
    C % 4 != 0 among them, batch 1 .. 3.  Blocks, 3 .. 5 per net, block seed % 7 of Q4OPS_BLOCKS always among them:
      instnorm    conv -> instance norm -> [add residual] -> [relu]
      pad         reflect / edge / constant pad (uneven sides; the constant 0 or 0.5, which with C % 4 != 0 has no channel-quad
                  form) -> conv with pads 0
      groupnorm   the five exporter steps (groupnorm_ref.five_steps) with C / G in {1, 2, 4, 8}, and 3, which stays NCHW,
                  -> [add residual] -> [relu]
      shuffle, unshuffle    the reshape / transpose / reshape trio (pixel_shuffle_ref.trio), r in {2, 3}, CRD and DCR; where the
                  last block is a shuffle it ends the program (nchw_out)
      linear      linear upsample x2 or resize to a size, alone or as the second term of an add (plan.fuse_linear_add); or a
                  nearest resize by whole scales or sizes, with a (transform, rounding) pair that has a channel-quad form or
                  one that shifts the map and stays NCHW (every third net also has one behind its first conv)
      dilated     3x3 convs with dilation 2 and 4 (plan.fold_dilated's heads) followed by relu / add / concat / a 1x1 conv (its
                  joins; a second add and its relu, which no conv's epilogue takes, run as steps on the folded tensors), with a
                  residual produced outside the fold, and dilation 2 -> 4 directly
    The input has per-channel magnitudes 2^U(-3, 3) and a DC offset, as random_net_real draws them.  -> (graph, blob, [x])"""
    from tests.groupnorm_ref import five_steps
    from tests.pixel_shuffle_ref import trio

    r = np.random.default_rng(seed)
    gb = GraphBuilder(["x"])

    class S:                                                            # what five_steps and trio write into
        g = gb

    n = int(r.choice([1, 2, 3]))
    c0 = int(r.choice([3, 4, 8]))
    h0, w0 = (int(v) for v in r.choice([10, 11, 12, 13, 14, 16, 18, 20], 2))
    gb.init("scales2", np.array([1, 1, 2, 2], np.float32))
    gb.init("roi", np.zeros(0, np.float32))
    gb.init("noscales", np.zeros(0, np.float32))
    uid = [0]

    def new(prefix):
        uid[0] += 1
        return "%s%d" % (prefix, uid[0])

    def conv(src, shape, cout, k=3, d=1, pads=None, bias=None, act="none"):
        c, h, w = shape
        K = gb.init(new("K"), (r.standard_normal((cout, c, k, k)) * np.sqrt(2.0 / (c * k * k))).astype(np.float32))
        ins = [src, K]
        if bias if bias is not None else r.random() < 0.5:
            ins.append(gb.init(new("B"), (r.standard_normal(cout) * 0.1).astype(np.float32)))
        p = [d * (k // 2)] * 4 if pads is None else pads
        cur = gb.op("conv", ins, new("c"), group=1, strides=[1, 1], dilations=[d, d], pads=p)
        if act == "relu":
            cur = gb.op("relu", cur, new("r"))
        return cur, (cout, h + p[0] + p[2] - d * (k - 1), w + p[1] + p[3] - d * (k - 1))

    def tail(cur, shape, res):
        """[add a residual of the same shape] -> [relu]"""
        if res is not None and r.random() < 0.6:
            cur = gb.op("add", [cur, res] if r.random() < 0.5 else [res, cur], new("a"))
        if r.random() < 0.6:
            cur = gb.op("relu", cur, new("r"))
        return cur

    def same_channels(cur, shape, like):
        return (cur, shape) if shape[0] == like else conv(cur, shape, like, k=1)

    def nearest(cur, shape, variant):
        """A nearest resize by whole factors, given as scales (variant < 3) or as sizes.  Of the (transform, rounding) pairs the
        first two do not shift the map and have a channel-quad form (plan.resize_nearest_q4_ok); the third shifts it by one
        pixel and stays NCHW."""
        c, h, w = shape
        fh, fw = [(2, 2), (1, 2), (2, 1)][int(r.integers(3))]
        trans, rounding = [("half_pixel", "round_prefer_floor"), ("asymmetric", "floor"), ("half_pixel", "floor")][variant % 3]
        if variant < 3:
            ins = [cur, "roi", gb.init(new("F"), np.array([1, 1, fh, fw], np.float32))]
        else:
            ins = [cur, "roi", "noscales", gb.init(new("Z"), np.array([0, 0, fh * h, fw * w], np.int64))]
        return (gb.op("resize", ins, new("u"), mode="nearest", coordinate_transformation_mode=trans, nearest_mode=rounding),
                (c, fh * h, fw * w))

    k = int(r.integers(3, 6))
    blocks = [Q4OPS_BLOCKS[seed % len(Q4OPS_BLOCKS)]] + [str(b) for b in r.choice(Q4OPS_BLOCKS, k - 1)]
    blocks = [blocks[i] for i in r.permutation(k)]
    cur, shape = conv("x", (c0, h0, w0), int(r.choice([4, 6, 8, 12, 16])), act="relu")
    if seed % 3 == 0:                                                   # every third net: a nearest resize, its six variants in turn
        cur, shape = nearest(cur, shape, seed // 3 % 6)
        cur, shape = conv(cur, shape, int(r.choice([4, 6, 8])), act="relu")
    for bi, kind in enumerate(blocks):
        c, h, w = shape
        last = bi == k - 1
        if kind == "shuffle" and max(h, w) * 2 > 40:
            kind = "unshuffle"
        if kind == "unshuffle" and not [q for q in (2, 3) if h % q == 0 and w % q == 0 and min(h, w) // q >= 5]:
            kind = "linear"
        if kind == "instnorm":
            co = c if r.random() < 0.6 else int(r.choice([4, 5, 8, 12, 18, 32, 64]))
            y, ys = conv(cur, shape, co)
            s = gb.init(new("s"), r.uniform(0.5, 1.5, co).astype(np.float32))
            t = gb.init(new("t"), (r.standard_normal(co) * 0.1).astype(np.float32))
            y = gb.op("instancenormalization", [y, s, t], new("n"), epsilon=1e-5)
            cur, shape = tail(y, ys, cur if co == c else None), ys
        elif kind == "pad":
            mode = str(r.choice(["reflect", "edge", "constant"]))
            pt, pl, pb, pr = (int(v) for v in r.integers(0, 3, 4))
            pads = gb.init(new("P"), np.array([0, 0, pt, pl, 0, 0, pb, pr], np.int64))
            para = {"mode": mode}
            if mode == "constant":              # 0.5 with a partial last quad: plan.pad_q4_ok declines, the pad stays NCHW
                para["constant_value"] = float(r.choice([0.0, 0.5]))
            y = gb.op("pad", [cur, pads], new("p"), **para)
            cur, shape = conv(y, (c, h + pt + pb, w + pl + pr), int(r.choice([4, 6, 8, 10, 16])), pads=[0, 0, 0, 0],
                              act=str(r.choice(["relu", "none"])))
        elif kind == "groupnorm":
            cpg = int(r.choice([1, 2, 4, 8, 3]))
            groups = int(r.choice([g for g in (1, 2, 3, 4, 6, 8) if 4 <= cpg * g <= 64]))
            co = cpg * groups
            y, ys = same_channels(cur, shape, co) if r.random() < 0.5 else conv(cur, shape, co)
            res = cur if co == c and y != cur else None
            y = five_steps(S, y, (1,) + ys, groups, tag=new("gn"), mid=str(r.choice(["3d", "4d"])),
                           affine=str(r.choice(["both", "both", "mul", "none"])), lead=bool(r.random() < 0.5), seed=seed * 100 + bi)
            cur, shape = tail(y, ys, res), ys
        elif kind == "shuffle":
            q, order = int(r.choice([2, 3])), str(r.choice(["crd", "dcr"]))
            if max(h, w) * q > 40:
                q = 2
            narrow = int(r.choice([3, 4, 5, 8] if order == "crd" else [4, 4, 8, 6]))
            y, ys = conv(cur, shape, narrow * q * q)
            cur = trio(S, y, (1,) + ys, q, order, False, tag=new("ps"))
            shape = (narrow, h * q, w * q)
            if last:                                                    # the shuffle ends the program
                break
            if r.random() < 0.5:
                cur, shape = conv(cur, shape, int(r.choice([4, 8, 12])), act="relu")
        elif kind == "unshuffle":
            q = int(r.choice([q for q in (2, 3) if h % q == 0 and w % q == 0 and min(h, w) // q >= 5]))
            order = str(r.choice(["crd", "dcr"]))
            if order == "dcr" and c % 4:
                cur, shape = conv(cur, shape, 4 * int(r.choice([1, 2])), k=1)
                c = shape[0]
            cur = trio(S, cur, (1,) + shape, q, order, True, tag=new("pu"))
            shape = (c * q * q, h // q, w // q)
            cur, shape = conv(cur, shape, int(r.choice([4, 8, 12, 16])), act="relu")
        elif kind == "linear":
            def up(src, tag):
                if how == "upsample":
                    return gb.op("upsample", [src, "scales2"], tag, mode="linear")
                size = gb.init(new("Z"), np.array([0, 0, oh, ow], np.int64))
                return gb.op("resize", [src, "roi", "noscales", size], tag, mode="linear",
                             coordinate_transformation_mode="half_pixel", nearest_mode="round_prefer_floor")
            how = "upsample" if max(h, w) * 2 <= 40 and r.random() < 0.5 else "resize"
            if max(h, w) * 2 <= 40 and r.random() < 0.3:
                how = "nearest"
            oh, ow = (2 * h, 2 * w) if how == "upsample" else (int(v) for v in r.integers(10, 41, 2))
            if how == "nearest":
                cur, (_, oh, ow) = nearest(cur, shape, int(r.integers(6)))
            elif r.random() < 0.5:
                a = up(cur, new("u"))
                b, _ = conv(cur, shape, c, k=1)
                cur = gb.op("add", [a, up(b, new("u"))], new("a"))      # the second term: fused into its upsample
            else:
                cur = up(cur, new("u"))
            shape = (c, oh, ow)
            cur, shape = conv(cur, shape, int(r.choice([4, 8, 10, 16])), act=str(r.choice(["relu", "none"])))
        else:                                                           # dilated
            if c % 4:
                cur, shape = conv(cur, shape, 4 * int(r.choice([1, 2, 3, 4])), k=1)
                c = shape[0]
            outside = cur                                               # produced outside the fold
            form = str(r.choice(["joins", "2to4", "alone"]))
            if form == "2to4":
                y, _ = conv(cur, shape, c, d=2)
                cur, _ = conv(y, shape, c, d=4, act=str(r.choice(["relu", "none"])))
            elif form == "alone":
                cur, shape = conv(cur, shape, int(r.choice([4, 6, 8])), d=int(r.choice([2, 4])))
            else:
                d = int(r.choice([2, 4]))
                first, _ = conv(cur, shape, c, d=d, act="relu")
                y, _ = conv(first, shape, c, d=d)
                y = gb.op("add", [y, outside], new("a"))
                y = gb.op("relu", y, new("r"))
                if r.random() < 0.6:                                    # steps no conv's epilogue takes: they run folded
                    y = gb.op("relu", gb.op("add", [y, first], new("a")), new("r"))
                if r.random() < 0.4:
                    y, shape = gb.op("concat", [y, first], new("k"), axis=1), (2 * c, h, w)
                cur, shape = conv(y, shape, int(r.choice([4, 8, 12])), k=1)
    g, blob = gb.finish([cur])
    x = r.standard_normal((n, c0, h0, w0)) * 2.0 ** r.uniform(-3, 3, (1, c0, 1, 1)) + float(r.choice([0.0, 4.0]))
    return g, blob, [x.astype(np.float32)]
