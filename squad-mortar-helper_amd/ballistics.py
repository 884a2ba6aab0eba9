"""Ballistics (include/smh_vision_hip.h, "ballistics"): a caller-supplied weapon and its firing solution on the host.  The library ships
no weapon table: Weapon() is the reference's mortar (smhv_weapon_defaults), everything else is the caller's."""
import ctypes as C
from dataclasses import dataclass

from . import _lib as L

_ARCS = {"high": L.ARC_HIGH, "low": L.ARC_LOW}
_UNITS = {"mils6400": L.ANGLE_MILS6400, "mils6000": L.ANGLE_MILS6000, "degrees": L.ANGLE_DEGREES}


@dataclass
class Weapon:
    """velocity m/s, gravity m/s^2 (the weapon's gravity scale multiplied in), arc "high" / "low" (the arc it is laid on), unit
    "mils6400" / "mils6000" / "degrees", elev_min / elev_max the mount's limits in that unit, range_min metres, dispersion the cone's
    half angle in radians.  The defaults are smhv_weapon_defaults'."""
    velocity: float = 109.890938
    gravity: float = 9.8
    arc: str = "high"
    unit: str = "mils6400"
    elev_min: float = 0.0
    elev_max: float = 1600.0
    range_min: float = 0.0
    dispersion: float = 0.0

    def struct(self):
        """-> smhv_weapon."""
        w = L.WeaponStruct()
        L.check(L.load().smhv_weapon_defaults(C.byref(w)))
        w.arc, w.unit = _ARCS[self.arc], _UNITS[self.unit]
        w.velocity, w.gravity = float(self.velocity), float(self.gravity)
        w.elev_min, w.elev_max = float(self.elev_min), float(self.elev_max)
        w.range_min, w.dispersion = float(self.range_min), float(self.dispersion)
        return w

    def check(self):
        """Raises VisionError for a weapon the library refuses (smhv_weapon_check)."""
        w = self.struct()
        L.check(L.load().smhv_weapon_check(C.byref(w)))

    def thresholds(self):
        """-> WeaponRule: V2, V4, the tangents of the limits and of the band edges (smhv_weapon_thresholds; host only)."""
        w, out = self.struct(), L.WeaponRule()
        L.check(L.load().smhv_weapon_thresholds(C.byref(w), C.byref(out)))
        return out


def solve(weapon, meters, alt=0.0):
    """The weapon's solution of one (meters, alt) on the host (smhv_ballistic_solve) -> BallisticSolution."""
    w, out = weapon.struct(), L.BallisticSolution()
    L.check(L.load().smhv_ballistic_solve(C.byref(w), float(meters), float(alt), C.byref(out)))
    return out
