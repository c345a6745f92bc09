"""NumPy restatement the PPO loss head tests compare against (no torch, no
library): the loss of the csrc/salp_ppo.hip header and its gradient in float64
with every per-row intermediate, the error bounds the float32 kernel is held
to, counted in float32 roundings of the reference's own intermediates, the
seeded input families of tests/test_gpu_ppo_loss.py, and the kernel's float32
log-prob in its own operation order.

Conventions (torch's): a tie of the minimum splits the gradient between its two
arguments, clamp passes the gradient on the closed interval, so a tie whose
ratio is inside [1 - c, 1 + c] passes the full advantage; no normalisation at
B == 1; std is the unbiased one."""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24                       # float32 unit roundoff
EPS64 = 2.0 ** -53
LOG_SQRT_2PI = 0.91893853320467274178
GRID, BLOCK = 256, 256               # csrc/salp_ppo.hip kPpoGrid, kPpoBlock
WORKSPACE_DOUBLES = 2048             # include/salp.h SALP_PPO_WORKSPACE_DOUBLES
UNCLIPPED, CLIPPED, TIE = 0, 1, 2    # which argument of the minimum is the smaller one
SCALARS = ("loss", "pg", "vf", "entropy", "clip_fraction")


def loss(mu, log_std, value, actions, old_logp, advantages, returns, clip_range, ent_coef, vf_coef,
         normalize_advantage):
    """float64 on the given (float32) arrays cast up.  Per row: logp, ratio, A
    (the advantage as used), branch (UNCLIPPED / CLIPPED / TIE), inside, dL_dr,
    dlogp; gradients dmu [B,3], dvalue [B], dlog_std [3]; the five scalars."""
    mu, ls, value, act, old, adv, ret = (np.asarray(x, np.float64) for x in
                                         (mu, log_std, value, actions, old_logp, advantages, returns))
    B = value.shape[0]
    var = np.exp(ls) ** 2
    d = act - mu
    t = d * d / (2 * var)                                  # [B,3]
    logp = (-t - ls - LOG_SQRT_2PI).sum(1)
    mean = std = None
    A = adv.copy()
    if normalize_advantage and B > 1:
        mean, std = adv.mean(), adv.std(ddof=1)
        A = (adv - mean) / (std + 1e-8)
    r = np.exp(logp - old)
    lo, hi = 1 - clip_range, 1 + clip_range
    rc = np.minimum(np.maximum(r, lo), hi)
    p1, p2 = A * r, A * rc
    branch = np.where(p1 < p2, UNCLIPPED, np.where(p2 < p1, CLIPPED, TIE))
    inside = (r >= lo) & (r <= hi)
    w1 = np.where(p1 < p2, 1.0, np.where(p1 == p2, 0.5, 0.0))
    w2 = np.where(p2 < p1, 1.0, np.where(p1 == p2, 0.5, 0.0))
    passes = (w1 > 0) | (inside & (w2 > 0))                # the row's gradient is not cut
    dL_dr = w1 * A + np.where(inside, w2 * A, 0.0)
    dlogp = -dL_dr * r / B                                 # d pg / d logp_b
    z = d * d / var
    dls_rows = dlogp[:, None] * (z - 1)
    e = ret - value
    pg, vf = -np.minimum(p1, p2).mean(), (e * e).mean()
    entropy = (0.5 + LOG_SQRT_2PI + ls).sum()
    return SimpleNamespace(
        B=B, ls=ls, var=var, d=d, t=t, z=z, old=old, adv=adv, mean=mean, std=std, logp=logp, ratio=r, rc=rc, A=A,
        branch=branch, inside=inside, passes=passes, dL_dr=dL_dr, dlogp=dlogp, e=e, dls_rows=dls_rows,
        dmu=dlogp[:, None] * d / var, dvalue=vf_coef * (-2 * e / B), dlog_std=dls_rows.sum(0) - ent_coef,
        loss=pg - ent_coef * entropy + vf_coef * vf, pg=pg, vf=vf, entropy=entropy,
        clip_fraction=(np.abs(r - 1) > clip_range).mean(), clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef)


def bounds(ref):
    """Error bounds of the float32 kernel against `ref`, first order in
    u = 2^-24, from ref's own intermediates (nothing the kernel computed).
    Counting the kernel's roundings (no contraction; expf within 1 ulp = 2 u):

    logp    per component t = d^2 / (2 var): d (1 u, twice), the square (1),
            expf (2, twice in sd^2), sd^2 (1), the division (1): 9 u t; then
            `- log_std`, `- log sqrt(2 pi)` and that constant's own rounding,
            each at most u T with T = t + |log_std| + 0.92, and the three
            accumulations, each at most u sum_j T:
              e_lp = u (9 sum t + 6 sum T)
    ratio   x = logp - old_logp rounds once (u (|logp| + |old_logp|)), and a
            relative error of exp(x) is an absolute error of x, plus expf:
              rho = e_lp + u (|logp| + |old_logp|) + 2 u        (relative)
    A       not normalised: exact.  Normalised: the float32 rounding of the
            mean moves adv - mean by u |mean|, i.e. A by  u |mean| / std;  the
            subtraction and the product by inv round once each (2 u |A|); inv =
            1 / ((float) sqrt(var) + 1e-8f) rounds three times (3 u) and takes
            half of var's relative error.  var = (q - s mean) / (B - 1) from
            fp64 sums: a term passes through at most D = passes + 6 (wave
            shuffles) + 4 (waves) + 256 (the fold over the blocks' partials)
            additions, then s / B, s mean and the subtraction, so var is off by
            2 (D + 3) 2^-53 q relative to q - s mean: kappa = q / sum (adv -
            mean)^2 is how much the one-pass formula amplifies (1 for centred
            advantages, 1e10 for 1e4 + 0.1 randn).
              e_A = u |mean| / std + |A| (5 u + (D + 3) 2^-53 kappa)
    dlogp   = -(1 / B) dL_dr r: 1 / B and two products (3 u); dL_dr is A on
            rows that pass the gradient (0.5 A + 0.5 A is exact) and exactly 0
            on cut rows:
              e_dlp = (e_A r + |dL_dr| r (rho + 3 u)) / B
    dmu     dlogp d / var: d (1), var (5), product, division: 8 u
              e_dmu = |d| / var (e_dlp + 8 u |dlogp|)       (0 on cut rows)
    dvalue  vf_coef (-2 e / B): e, 1 / B, its product, vf_coef's rounding and
            its product: 5 u |dvalue|
    dlog_std  row term dlogp (z - 1), z = d^2 / var (9 u z as t above), the
            subtraction and the product (2 u |z - 1|); the fp64 sum of B float32
            terms adds B 2^-53 sum |term|; (float) sum, ent_coef's rounding and
            the subtraction round once each:
              sum_b [e_dlp |z - 1| + |dlogp| (9 u z + 2 u |z - 1|)] + u (|S| + |ent_coef| + |S - ent_coef|)
    pg      row term min(A r, A rc): min is 1-Lipschitz in both arguments, the
            clip edges 1 -+ (float) c are within 2 u of the float64 ones, the
            product rounds once: e_A R + |A| R (rho + 3 u), R = max(r, rc);
            the mean of the row bounds plus (float)'s rounding u |pg|
    vf      e^2: 2 u from e, 1 from the square; mean, then (float): 4 u vf
    entropy three additions of ((0.5 + 0.92) + log_std_j): the constant (2 u:
            0.92's rounding and the sum's), the inner sum and the running sum
    loss    pg - ent_coef ent + vf_coef vf: the terms' own errors, each
            coefficient's rounding and product (2 u), two additions (2 u of the
            magnitudes' sum)
    margin  how far a ratio must be from 1 -+ c for float32 and float64 to
            agree on its side: r rho, r - 1's rounding and (float) c's: below
            r rho + 4 u (1 + c)."""
    B, r, A = ref.B, ref.ratio, np.abs(ref.A)
    T = ref.t + np.abs(ref.ls) + LOG_SQRT_2PI
    e_lp = U * (9 * ref.t.sum(1) + 6 * T.sum(1))
    rho = e_lp + U * (np.abs(ref.logp) + np.abs(ref.old)) + 2 * U
    e_A = np.zeros(B)
    if ref.mean is not None:
        depth = -(-B // (GRID * BLOCK)) + 6 + 4 + GRID
        kappa = (ref.adv ** 2).sum() / ((ref.adv - ref.mean) ** 2).sum()
        e_A = U * abs(ref.mean) / ref.std + A * (5 * U + (depth + 3) * EPS64 * kappa)
    absdL, absdlp = np.abs(ref.dL_dr), np.abs(ref.dlogp)
    e_dlp = (np.where(ref.passes, e_A, 0.0) * r + absdL * r * (rho + 3 * U)) / B
    dz = np.abs(ref.z - 1)
    ec, vc = abs(ref.ent_coef), abs(ref.vf_coef)
    S = ref.dls_rows.sum(0)
    R = np.maximum(r, ref.rc)
    c0 = 0.5 + LOG_SQRT_2PI
    run = np.cumsum(c0 + ref.ls)
    e_ent = (2 * U * c0 + U * np.abs(c0 + ref.ls)).sum() + U * np.abs(run[1:]).sum()
    e_pg = (e_A * R + A * R * (rho + 3 * U)).mean() + U * abs(ref.pg) + B * EPS64 * np.abs(A * R).mean()
    e_vf = 4 * U * ref.vf
    return SimpleNamespace(
        dmu=np.abs(ref.d) / ref.var * (e_dlp + 8 * U * absdlp)[:, None],
        dvalue=5 * U * np.abs(ref.dvalue),
        dlog_std=((e_dlp[:, None] * dz + absdlp[:, None] * (9 * U * ref.z + 2 * U * dz)).sum(0)
                  + U * (np.abs(S) + ec + np.abs(S - ref.ent_coef)) + B * EPS64 * np.abs(ref.dls_rows).sum(0)),
        pg=e_pg, vf=e_vf, entropy=e_ent,
        loss=(e_pg + ec * (e_ent + 2 * U * abs(ref.entropy)) + vc * (e_vf + 2 * U * ref.vf)
              + 2 * U * (abs(ref.pg) + ec * abs(ref.entropy) + vc * ref.vf)),
        margin=r * rho + 4 * U * (1 + ref.clip_range))


def sides_are_decided(ref, bnd):
    """The precondition of the exact clip_fraction (and of equal branches):
    every ratio is further than its margin from both 1 - c and 1 + c."""
    c = ref.clip_range
    return bool((np.minimum(np.abs(ref.ratio - (1 - c)), np.abs(ref.ratio - (1 + c))) > bnd.margin).all())


def worst(got, ref, bnd):
    """{tensor: worst error / bound}; `got` maps names to the kernel's arrays
    (out[8] split into the scalars and dlog_std).  A bound of 0 asks for an
    exact 0 (inf otherwise).  clip_fraction: 0 if it is float32(ref)'s bits."""
    out = {}
    for name in ("dmu", "dvalue", "dlog_std", "loss", "pg", "vf", "entropy"):
        err = np.abs(np.asarray(got[name], np.float64) - getattr(ref, name))
        b = np.broadcast_to(np.asarray(getattr(bnd, name), np.float64), err.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
        out[name] = float(np.max(ratio))
    out["clip_fraction"] = 0.0 if np.float32(got["clip_fraction"]) == np.float32(ref.clip_fraction) else np.inf
    return out


def split_out(out8):
    """out[8] of salp_ppo_loss -> the five scalars and dlog_std."""
    got = dict(zip(SCALARS, (float(v) for v in out8[:5])))
    got["dlog_std"] = np.asarray(out8[5:8])
    return got


# ------------------------------------------------------------ kernel's float32
def logp_f32(mu, log_std, actions):
    """The kernel's log-prob in float32, operation for operation (no
    contraction): lp += ((-(d d)) / (2 var) - log_std) - log sqrt(2 pi)."""
    f = np.float32
    mu, ls, act = (np.asarray(x, f) for x in (mu, log_std, actions))
    sd = np.exp(ls)
    var = sd * sd
    lp = np.zeros(mu.shape[0], f)
    for j in range(3):
        d = act[:, j] - mu[:, j]
        lp = lp + ((-(d * d)) / (f(2) * var[j]) - ls[j] - f(LOG_SQRT_2PI))
    return lp


# --------------------------------------------------------------- input families
def generic(B, seed, ratio_spread=0.3, log_std=None):
    """The recipe of test_fused_loss_matches_torch's _case on a seeded CPU
    generator: (mu, log_std, value, actions, old_logp, advantages, returns)."""
    g = np.random.default_rng(seed)
    r = g.standard_normal
    f = np.float32
    mu = (r((B, 3)) * 0.5).astype(f)
    ls = (r(3) * 0.3).astype(f) if log_std is None else np.asarray(log_std, f)
    value = (r(B) * 10).astype(f)
    act = (mu + r((B, 3)) * np.exp(ls.astype(np.float64))).astype(f)
    d = act.astype(np.float64) - mu
    lp = (-d * d / (2 * np.exp(ls.astype(np.float64)) ** 2) - ls - LOG_SQRT_2PI).sum(1)
    old = (lp + r(B) * ratio_spread).astype(f)              # ratios around 1, some clipped
    adv = (r(B) * 100 + 3).astype(f)
    ret = (value + r(B) * 5).astype(f)
    return [mu, ls, value, act, old, adv, ret]


def far_advantages(B, seed, kind):
    """generic() with advantages far from zero: 'e3' 1e3 + randn, 'e4' 1e4 +
    0.1 randn, 'equal' all 1234.5 (std 0: the normalised advantage is 0)."""
    a = generic(B, seed)
    g = np.random.default_rng(seed + 1000)
    a[5] = {"e3": 1e3 + g.standard_normal(B), "e4": 1e4 + 0.1 * g.standard_normal(B),
            "equal": np.full(B, 1234.5)}[kind].astype(np.float32)
    return a


def clipped_rows(B, seed, clip_range=0.2):
    """Rows in five kinds, row b of kind b % 5, ratios 1.5 or 0.5 (well outside
    1 -+ 0.2): 0: A > 0, r = 1.5 (cut), 1: A < 0, r = 0.5 (cut), 2: A < 0,
    r = 1.5 (passes), 3: A > 0, r = 0.5 (passes), 4: A == 0 (r = 1.5)."""
    a = generic(B, seed)
    kind = np.arange(B) % 5
    ref = loss(*a, clip_range, 0.0, 0.5, False)
    target = np.where((kind == 1) | (kind == 3), 0.5, 1.5)
    a[4] = (ref.logp - np.log(target)).astype(np.float32)
    mag = np.abs(a[5]) + 1
    a[5] = np.select([kind == 4, (kind == 0) | (kind == 3)], [0.0, mag], -mag).astype(np.float32)
    return a, kind


def convention_rows(B, seed):
    """log_std = 0, mu and actions on multiples of 1/8, advantages signed
    powers of two and old_logp the kernel's own float32 log-prob: every ratio
    is exactly 1, and with B a power of two -A d / B is exact in float32."""
    g = np.random.default_rng(seed)
    f = np.float32
    mu = (g.integers(-8, 9, (B, 3)) / 8).astype(f)
    act = (mu + g.integers(-12, 13, (B, 3)) / 8).astype(f)
    adv = (g.choice([-1.0, 1.0], B) * 2.0 ** g.integers(-2, 3, B)).astype(f)
    ls = np.zeros(3, f)
    value = (g.integers(-16, 17, B) / 4).astype(f)
    ret = (value + g.integers(-8, 9, B) / 4).astype(f)
    return [mu, ls, value, act, logp_f32(mu, ls, act), adv, ret]


def settle(args, clip_range, normalize, tries=8):
    """Move old_logp of the rows whose float64 ratio is within twice the margin
    of a clip edge by 1/32 (about 3 % of the ratio), until none is left."""
    args = list(args)
    for _ in range(tries):
        ref = loss(*args, clip_range, 0.0, 0.5, normalize)
        m = 2 * bounds(ref).margin
        near = np.minimum(np.abs(ref.ratio - (1 - clip_range)), np.abs(ref.ratio - (1 + clip_range))) <= m
        if not near.any():
            return args
        args[4] = np.where(near, args[4] + np.float32(1 / 32), args[4]).astype(np.float32)
    raise AssertionError("settle: ratios stay near a clip edge")
