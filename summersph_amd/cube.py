"""Position-position-velocity cubes of a save file on the GPU (sph_cube): the viewing matrix, the channel axis, moments,
position-velocity cuts and a FITS writer around Context.cube.

    python -m summersph_amd.cube save275.txt -o cube.npz --inc 40 --pa 30 --extent 200 --size 256 --vrange -5 5 --nchan 64 \\
        --sigma-scale 0.3 --fits cube.fits --json

Conventions.  The rows of the viewing matrix are the image axes u^, v^ and the line of sight w^.  w^ points AWAY from the
observer, so a positive line-of-sight velocity is receding (red-shifted).  view(0, 0) is the identity: the observer looks
down the z axis onto the x-y plane, u^ = x^, v^ = y^.  The disc is first turned by `azimuth` about z, then tilted by
`inclination` about u^ (the line of nodes), then the image is turned by `position_angle` about the line of sight."""
import argparse
import json
import sys

import numpy as np

from .cli import read_save, uploaded_context


def view(inclination, position_angle=0.0, azimuth=0.0):
    """The 3 x 3 matrix rot (rows u^, v^, w^) of a view inclined by `inclination` degrees (0: face-on, w^ = z^; 90: edge-on,
    z^ in the image plane) whose line of nodes makes the angle `position_angle` (degrees) with the image's u axis, of a
    disc turned by `azimuth` degrees about z.  Orthonormal, right-handed."""
    i, pa, az = (np.deg2rad(float(a)) for a in (inclination, position_angle, azimuth))
    rz = np.array([[np.cos(az), np.sin(az), 0.0], [-np.sin(az), np.cos(az), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(i), np.sin(i)], [0.0, -np.sin(i), np.cos(i)]])
    rw = np.array([[np.cos(pa), -np.sin(pa), 0.0], [np.sin(pa), np.cos(pa), 0.0], [0.0, 0.0, 1.0]])
    r = rw @ rx @ rz
    # Gram-Schmidt in double precision: the products above are orthonormal to a few ulp, sph_cube asks for 1e-12
    u = r[0] / np.linalg.norm(r[0])
    v = r[1] - np.dot(r[1], u) * u
    v /= np.linalg.norm(v)
    return np.stack([u, v, np.cross(u, v)])


def channels(v0, dv, n):
    """The centres v0 + k dv of the n channels (channel k spans (k - 0.5) dv + v0 .. (k + 0.5) dv + v0)"""
    if n < 1 or not dv > 0:
        raise ValueError("channels: n >= 1 and dv > 0")
    return float(v0) + float(dv) * np.arange(int(n))


def vrange_channels(v_lo, v_hi, n):
    """(v0, dv) of n channels whose edges span v_lo .. v_hi"""
    if not v_hi > v_lo or n < 1:
        raise ValueError("vrange: lo < hi and nchan >= 1")
    dv = (float(v_hi) - float(v_lo)) / int(n)
    return float(v_lo) + 0.5 * dv, dv


def moments(cube, v):
    """(m0, m1, m2, peak) of a cube of shape (n_chan, ...) over the channel centres v: m0 = sum_k I_k, m1 = sum I_k v_k /
    m0 (the intensity-weighted mean velocity), m2 = sqrt(sum I_k (v_k - m1)^2 / m0) (the dispersion) and the centre of
    the brightest channel; m1, m2 and peak are NaN where m0 == 0."""
    cube = np.asarray(cube, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64).reshape((-1,) + (1,) * (cube.ndim - 1))
    if v.shape[0] != cube.shape[0]:
        raise ValueError("moments: one velocity per channel")
    m0 = cube.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        m1 = (cube * v).sum(axis=0) / m0
        m2 = np.sqrt(np.maximum((cube * (v - m1) ** 2).sum(axis=0) / m0, 0.0))
    peak = np.where(m0 != 0.0, v.reshape(-1)[np.argmax(cube, axis=0)], np.nan)
    bad = m0 == 0.0
    m1 = np.where(bad, np.nan, m1)
    m2 = np.where(bad, np.nan, m2)
    return m0, m1, m2, peak


def pv_cut(cube, bounds, p0, p1, n):
    """The position-velocity diagram along the slit from image point p0 = (u, v) to p1: (pv (n_chan, n), offsets (n,)),
    the cube interpolated bilinearly between its nodes at n equidistant points; offsets are distances from p0.  Points
    outside the node box are NaN."""
    cube = np.asarray(cube, dtype=np.float64)
    (lo_u, lo_v), (hi_u, hi_v) = bounds
    _, n_u, n_v = cube.shape
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    s = np.linspace(0.0, 1.0, int(n))
    pts = p0[None, :] + s[:, None] * (p1 - p0)[None, :]

    def frac(x, lo, hi, nn):
        if nn == 1:
            return np.zeros_like(x), np.zeros(x.shape, dtype=int), np.isclose(x, lo)
        f = (x - lo) / (hi - lo) * (nn - 1)
        ok = (f >= 0.0) & (f <= nn - 1)
        i = np.clip(np.floor(f).astype(int), 0, nn - 2)
        return f - i, i, ok

    fu, iu, oku = frac(pts[:, 0], lo_u, hi_u, n_u)
    fv, iv, okv = frac(pts[:, 1], lo_v, hi_v, n_v)
    iu1, iv1 = np.minimum(iu + 1, n_u - 1), np.minimum(iv + 1, n_v - 1)
    pv = (cube[:, iu, iv] * (1 - fu) * (1 - fv) + cube[:, iu1, iv] * fu * (1 - fv) + cube[:, iu, iv1] * (1 - fu) * fv +
          cube[:, iu1, iv1] * fu * fv)
    pv[:, ~(oku & okv)] = np.nan
    return pv, s * float(np.linalg.norm(p1 - p0))


def _card(key, value, comment=""):
    if isinstance(value, bool):
        val = f"{'T' if value else 'F':>20}"
    elif isinstance(value, (int, np.integer)):
        val = f"{int(value):>20d}"
    elif isinstance(value, (float, np.floating)):
        val = f"{float(value):>20.16E}"
    else:
        val = f"'{str(value):<8}'"
        val = f"{val:<20}"
    card = f"{key:<8}= {val}" + (f" / {comment}" if comment else "")
    return f"{card[:80]:<80}"


def write_fits(path, cube, bounds, v0, dv, bunit="", extra=None):
    """A dependency-free FITS file of the cube: one primary HDU, BITPIX -64, big-endian, 2880-byte blocks.  FITS axis 1
    (fastest) is the image's v axis, axis 2 the u axis, axis 3 the velocity, each with a linear CRPIX / CRVAL / CDELT (a
    single node has CDELT 1).  extra: further (key, value, comment) cards."""
    cube = np.asarray(cube, dtype=np.float64)
    if cube.ndim != 3:
        raise ValueError("write_fits: a cube of shape (n_chan, n_u, n_v)")
    n_chan, n_u, n_v = cube.shape
    (lo_u, lo_v), (hi_u, hi_v) = bounds

    def step(lo, hi, n):
        return (float(hi) - float(lo)) / (n - 1) if n > 1 else 1.0
    cards = [_card("SIMPLE", True, "conforms to FITS"), _card("BITPIX", -64, "IEEE double"), _card("NAXIS", 3),
             _card("NAXIS1", n_v), _card("NAXIS2", n_u), _card("NAXIS3", n_chan)]
    for ax, (name, ref, delt) in enumerate((("V", lo_v, step(lo_v, hi_v, n_v)), ("U", lo_u, step(lo_u, hi_u, n_u)),
                                            ("VELO", v0, dv)), start=1):
        cards += [_card(f"CTYPE{ax}", name), _card(f"CRPIX{ax}", 1.0), _card(f"CRVAL{ax}", float(ref)),
                  _card(f"CDELT{ax}", float(delt))]
    if bunit:
        cards.append(_card("BUNIT", bunit))
    for key, value, comment in (extra or ()):
        cards.append(_card(key, value, comment))
    cards.append(f"{'END':<80}")
    header = "".join(cards).encode("ascii")
    header += b" " * (-len(header) % 2880)
    data = np.ascontiguousarray(cube, dtype=">f8").tobytes()
    data += b"\0" * (-len(data) % 2880)
    with open(path, "wb") as f:
        f.write(header)
        f.write(data)


def read_fits(path):
    """(header dict, data) of a file written by write_fits (primary HDU of doubles only)"""
    raw = open(path, "rb").read()
    hdr, pos, done = {}, 0, False
    while not done:
        block = raw[pos:pos + 2880].decode("ascii")
        pos += 2880
        for k in range(0, 2880, 80):
            card = block[k:k + 80]
            if card.startswith("END"):
                done = True
                break
            if card[8:10] != "= ":
                continue
            val = card[10:].split(" / ")[0].strip()
            if val.startswith("'"):
                hdr[card[:8].strip()] = val.strip("'").rstrip()
            elif val in ("T", "F"):
                hdr[card[:8].strip()] = val == "T"
            else:
                hdr[card[:8].strip()] = float(val) if any(ch in val for ch in ".E") else int(val)
    shape = tuple(hdr[f"NAXIS{a}"] for a in range(hdr["NAXIS"], 0, -1))
    n = int(np.prod(shape))
    return hdr, np.frombuffer(raw, dtype=">f8", count=n, offset=pos).reshape(shape).astype(np.float64)


def parse_vec(s, n=3):
    v = tuple(float(t) for t in s.split(","))
    if len(v) != n:
        raise ValueError(f"{s!r}: {n} comma-separated numbers")
    return v


def parse_clip(s):
    v = parse_vec(s, 6)
    return (v[:3], v[3:])


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m summersph_amd.cube", description=__doc__.split("\n\n")[0])
    ap.add_argument("save", help="save file")
    ap.add_argument("-o", "--out", required=True, help="output .npz (cube, v, u_nodes, v_nodes, rot, moment0 .. 2, peak)")
    ap.add_argument("--variable", action="store_true", help="10-value gas records (.. alpha h), variable-h context")
    ap.add_argument("--inc", type=float, default=0.0, help="inclination in degrees (0: face-on)")
    ap.add_argument("--pa", type=float, default=0.0, help="position angle of the line of nodes in degrees")
    ap.add_argument("--azimuth", type=float, default=0.0, help="turn of the disc about z in degrees")
    ap.add_argument("--extent", type=float, required=True, help="full width of the square image (centred on --centre)")
    ap.add_argument("--size", type=int, default=256, help="image nodes per axis")
    ap.add_argument("--vrange", nargs=2, type=float, required=True, metavar=("VLO", "VHI"), help="velocity range the channels span")
    ap.add_argument("--nchan", type=int, default=64, help="channels")
    ap.add_argument("--sigma-scale", type=float, default=0.0, help="line width in units of each particle's sound speed")
    ap.add_argument("--sigma-floor", type=float, default=0.0, help="line width added in quadrature")
    ap.add_argument("--centre", default="0,0,0", help="image centre x,y,z")
    ap.add_argument("--vref", default="0,0,0", help="reference velocity vx,vy,vz")
    ap.add_argument("--h", type=float, default=None, help="one h for every particle (default: each particle's own)")
    ap.add_argument("--clip", default=None, help="strict particle clip box x0,y0,z0,x1,y1,z1")
    ap.add_argument("--per-velocity", action="store_true", help="divide the channels by their width")
    ap.add_argument("--fits", default=None, help="also write the cube as a FITS file")
    ap.add_argument("--json", action="store_true", help="print a one-line JSON summary")
    ap.add_argument("--device", type=int, default=0)
    return ap


def args_desc(a):
    """Context.cube's keyword arguments from the parsed command line"""
    if a.size < 1 or a.nchan < 1:
        raise ValueError("--size and --nchan must be >= 1")
    if not (np.isfinite(a.extent) and a.extent > 0):
        raise ValueError("--extent must be finite and > 0")
    if a.h is not None and not (np.isfinite(a.h) and a.h > 0):
        raise ValueError("--h must be finite and > 0")
    if a.sigma_scale < 0 or a.sigma_floor < 0:
        raise ValueError("--sigma-scale and --sigma-floor must be >= 0")
    v0, dv = vrange_channels(a.vrange[0], a.vrange[1], a.nchan)
    half = 0.5 * a.extent
    return dict(shape=(a.size, a.size), bounds=((-half, -half), (half, half)), v0=v0, dv=dv, n_chan=a.nchan,
                rot=view(a.inc, a.pa, a.azimuth), centre=parse_vec(a.centre), v_ref=parse_vec(a.vref),
                sigma_scale=a.sigma_scale, sigma_floor=a.sigma_floor, h=a.h,
                clip=None if a.clip is None else parse_clip(a.clip), per_velocity=a.per_velocity)


def cube_rows(gas, sinks, kw, variable=False, device=0):
    """Uploads the rows into a fresh context and returns its cube (Context.cube(**kw))."""
    with uploaded_context(gas, sinks, variable, device) as ctx:
        if kw.get("sigma_scale", 0.0) != 0.0:
            ctx.density()                   # the sound speed c
        return ctx.cube(**kw)


def main(argv=None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    try:
        kw = args_desc(a)
    except ValueError as e:
        ap.error(str(e))
    gas, sinks = read_save(a.save, a.variable)
    cube = cube_rows(gas, sinks, kw, a.variable, a.device)
    v = channels(kw["v0"], kw["dv"], kw["n_chan"])
    m0, m1, m2, peak = moments(cube, v)
    (lo_u, lo_v), (hi_u, hi_v) = kw["bounds"]
    np.savez(a.out, cube=cube, v=v, u_nodes=np.linspace(lo_u, hi_u, a.size), v_nodes=np.linspace(lo_v, hi_v, a.size),
             rot=kw["rot"], moment0=m0, moment1=m1, moment2=m2, peak=peak, v0=np.array(kw["v0"]), dv=np.array(kw["dv"]))
    if a.fits:
        write_fits(a.fits, cube, kw["bounds"], kw["v0"], kw["dv"],
                   extra=[("INCL", float(a.inc), "inclination [deg]"), ("POSANG", float(a.pa), "position angle [deg]")])
    seen = m0 > 0
    summary = {"shape": list(cube.shape), "total": float(cube.sum()) * (kw["dv"] if a.per_velocity else 1.0),
               "pixels_lit": int(seen.sum()), "v_mean_abs_max": float(np.nanmax(np.abs(m1))) if seen.any() else None}
    if a.json:
        print(json.dumps(summary))
    else:
        print(f"{a.out}: cube {cube.shape} from {gas.shape[0]} gas rows, {summary['pixels_lit']} pixels lit")
    return 0


if __name__ == "__main__":
    sys.exit(main())
