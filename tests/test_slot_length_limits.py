"""The ends of the slot-length axis, on the host: the ``Simulation`` shell refuses a ``TimePeriods`` that is not a whole number of
minutes (it used to run 90-second slots as one-minute slots, and 30 seconds failed later with an unrelated message), ``vds_create``
refuses a slot length beyond VDS_TICK_MINUTES_MAX.  Nothing here is launched.  (The builder's refusal of a day whose minutes do not
fit int32: tests/test_order_tables.py.)"""
import datetime as dt

import numpy as np
import pandas as pd
import pytest

from test_order_tables import TICK_MINUTES_MAX
from vehicles_dispatch_simulator_amd import BatchedDispatchEnv
from vehicles_dispatch_simulator_amd.simulation import Simulation, slot_minutes


def shell(time_periods):
    return Simulation(ClusterMode="Grid", DemandPredictionMode="None", DispatchMode="Simulation", VehiclesNumber=10, TimePeriods=time_periods,
                      LocalRegionBound=(104.011, 104.125, 30.618, 30.703), SideLengthMeter=800, VehiclesServiceMeter=800,
                      NeighborCanServer=False, FocusOnLocalRegion=False, Quiet=True)


@pytest.mark.parametrize("value", [np.timedelta64(90, "s"), np.timedelta64(30, "s"), np.timedelta64(0, "m"), pd.Timedelta(seconds=61),
                                   dt.timedelta(minutes=-10), np.timedelta64(90 * 10**9)], ids=["90s", "30s", "0", "61s", "-10min", "90e9ns"])
def test_time_periods_that_are_not_whole_minutes_are_refused(value):
    with pytest.raises(ValueError, match="slots are whole minutes here") as e:
        shell(value)
    assert repr(value) in str(e.value)


@pytest.mark.parametrize("value,minutes", [(np.timedelta64(1, "m"), 1), (np.timedelta64(600 * 10**9), 10), (dt.timedelta(hours=24), 1440)])
def test_whole_minutes_are_taken(value, minutes):
    """``slot_minutes`` is what the constructor checks with and what every load hands to the engine as ``tick_minutes``."""
    sim = shell(value)
    assert sim.TimePeriods is value and slot_minutes(sim.TimePeriods) == minutes


def test_vds_create_refuses_a_slot_length_beyond_the_bound():
    cost = np.zeros((2, 2), np.int32)
    with pytest.raises(Exception, match=r"vds_create failed \(-1\): vds_create: tick_minutes %d > %d" % (TICK_MINUTES_MAX + 1, TICK_MINUTES_MAX)):
        BatchedDispatchEnv(cost, np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(0, np.int32), replicas=1, vehicles=1,
                           tick_minutes=TICK_MINUTES_MAX + 1)
