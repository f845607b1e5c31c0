/* myo_hip_sensors.h -- touch sensors and contact forces of the HIP stepper (included by myo_hip.h; not a stand-alone header).
 * An extension of libmyo_hip.so only: the float64 oracle's twin of the ABI (oracle/myo_oracle_abi.c) has no counterpart, the oracle side of
 * the sensor check is tests/touch_ref.py on the oracle's own contacts and constraint forces. */
#ifndef MYO_HIP_SENSORS_H
#define MYO_HIP_SENSORS_H

/* number of sensors of the compiled model (touch sensors; 0: none, or a blob compiled before sensors were) */
int myo_model_nsensor(const myo_model*);
/* Allocates MYO_F_SENSORDATA / MYO_F_CFRC and turns on their readout in the step kernel (one uniform branch per launch when off).
 * MYO_E_UNSUPPORTED, with the cause in myo_last_error(), for a model without touch sensors (no hip_touch table in the blob), a model of
 * the hand class, the TrackEnv class or with the RK4 integrator, and when lanes != 64 (myo_set_lanes).  Idempotent */
int myo_batch_enable_sensors(myo_batch*);

#endif
