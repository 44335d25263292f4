# PigeonMI355X.jl — the binding a Pigeon.jl maintainer would add to drive the MI355X hot path (libpigeon_hip.so) from Julia.
#
# NOT EXECUTED in the build container (no Julia toolchain there); the same C ABI is exercised by the Python mirror
# (pigeon.jl_amd/mpc.py) and by tests/.  Function names and call order are the reference's own
# (src/model_predictive_control.jl:70-78); `mpc` is a batch of B independent controllers instead of one.
module PigeonMI355X

using StaticArrays
import Pigeon
import Pigeon: compute_time_steps!, compute_linearization_nodes!, update_QP!, get_next_control,
               BicycleState, BicycleControl, SimpleCarState, TrajectoryTube, CoupledControlParams, X1
import Parametron: solve!

# libpigeon_hip.so computes in Float64 (the reference's type); libpigeon_hip_f32.so is the same translation unit instantiated for Float32, same ABI
# (host arrays stay Float64; only device arrays handed to the *_dev entry points change element type).  The library is chosen PER CONTROLLER
# (keyword `precision = :f64 | :f32`), so the symbols are resolved through Libdl instead of a constant library name.
using Libdl
const LIBDIR = get(ENV, "PIGEON_HIP_LIBDIR", joinpath(@__DIR__, "..", "pigeon.jl_amd", "csrc"))
const LIBS = Dict{Symbol,Ptr{Cvoid}}()
function lib(precision::Symbol)
    get!(LIBS, precision) do
        h = Libdl.dlopen(joinpath(LIBDIR, precision == :f32 ? "libpigeon_hip_f32.so" : "libpigeon_hip.so"))
        check_layout(h)
        ccall(Libdl.dlsym(h, :pg_precision_bits), Cint, ()) == (precision == :f32 ? 32 : 64) || error("library / precision mismatch")
        h
    end
end

# mirrors of the C structs of include/pigeon_mpc.h (isbits, same field order)
struct PgVehicle
    G::Float64; m::Float64; Izz::Float64; L::Float64; a::Float64; b::Float64; h::Float64; mu::Float64; Caf::Float64; Car::Float64
    Cd0::Float64; Cd1::Float64; Cd2::Float64; fwd_frac::Float64; rwd_frac::Float64; fwb_frac::Float64; rwb_frac::Float64
    Fx_max::Float64; Fx_min::Float64; Px_max::Float64; delta_max::Float64; kappa_max::Float64
end
struct PgControlParams
    V_min::Float64; V_max::Float64; k_V::Float64; k_s::Float64; deltadot_max::Float64
    Q_ds::Float64; Q_dpsi::Float64; Q_e::Float64; W_beta::Float64; W_r::Float64; W_HJI::Float64
    R_delta::Float64; R_ddelta::Float64; R_Fx::Float64; R_dFx::Float64
    N_HJI::Int32; _pad::Int32
end
struct PgConfig
    vehicle::PgVehicle
    control::PgControlParams
    N_short::Int32
    N_long::Int32
    dt_short::Float64
    dt_long::Float64
    use_correction_step::Int32
    rk4_substeps::Int32
    hji_eps::Float64
    batch_capacity::Int32
    device::Int32
    ipm_max_iter::Int32
    formulation::Int32          # 0 coupled (src/coupled_lat_long.jl), 1 decoupled (src/decoupled_lat_long.jl)
    ipm_tol::Float64
    ipm_mu0::Float64
    walls::Int32                # build-defined soft wall rows (decoupled only)
    allow_f32_long_lateral::Int32   # fp32 library only: 1 = accept the decoupled formulation beyond 32 intervals (refused otherwise: steering up to 6e-3 rad off at N = 50)
    wall_weight::Float64
    polish::Int32               # active-set polish after the interior point
    _pad3::Int32
    polish_rho::Float64
    polish_tol::Float64
    polish_ipm_tol::Float64
    warm_polish::Int32          # previous active set + multipliers as the polish's first guess (the counterpart of OSQP's warm start)
    cold_guess::Int32           # rounds a cold instance may spend on the polish started from the empty active set before the interior point runs (0 = off)
end

"The structs above are a hand copy of include/pigeon_mpc.h: compare their layout with what the library was compiled with (pg_abi_layout) before the first pg_create."
function check_layout(h)
    n = ccall(Libdl.dlsym(h, :pg_abi_layout), Cint, (Ptr{Int32}, Int32), C_NULL, 0)
    theirs = Vector{Int32}(undef, n)
    ccall(Libdl.dlsym(h, :pg_abi_layout), Cint, (Ptr{Int32}, Int32), theirs, n)
    off(f) = Int32(fieldoffset(PgConfig, Base.fieldindex(PgConfig, f)))
    mine = Int32[sizeof(PgConfig), sizeof(PgVehicle), sizeof(PgControlParams),
                 off(:control), off(:N_short), off(:dt_short), off(:use_correction_step), off(:hji_eps), off(:batch_capacity), off(:ipm_max_iter), off(:formulation),
                 off(:ipm_tol), off(:ipm_mu0), off(:walls), off(:wall_weight), off(:polish), off(:polish_rho), off(:polish_tol), off(:polish_ipm_tol), off(:warm_polish), off(:cold_guess),
                 fieldoffset(PgControlParams, Base.fieldindex(PgControlParams, :N_HJI)), fieldoffset(PgVehicle, Base.fieldindex(PgVehicle, :kappa_max))]
    mine == theirs || error("PigeonMI355X.jl struct layout $mine differs from the library's $theirs: update the mirrors to include/pigeon_mpc.h")
end

check(mpc, rc, what) = rc == 0 || error("$what failed ($rc): " * unsafe_string(ccall(Libdl.dlsym(mpc.lib, :pg_last_error), Cstring, (Ptr{Cvoid},), mpc.handle)))
sym(mpc, name::Symbol) = Libdl.dlsym(mpc.lib, name)

"B copies of CoupledTrajectoryTrackingMPC / DecoupledTrajectoryTrackingMPC (src/coupled_lat_long.jl:42-60, src/decoupled_lat_long.jl:32-50) on one MI355X."
mutable struct BatchedTrajectoryTrackingMPC
    lib::Ptr{Cvoid}
    handle::Ptr{Cvoid}
    B::Int
    current_state::Vector{BicycleState{Float64}}        # fields the ROS callback writes (src/ros_integration.jl:50-53)
    current_control::Vector{BicycleControl{Float64}}
    other_car_state::Vector{SimpleCarState{Float64}}
    time_offset::Vector{Float64}
    t::Vector{Float64}
end

function _create(cfg::PgConfig, L::Ptr{Cvoid}, trajectory, B)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall(Libdl.dlsym(L, :pg_create), Cint, (Ref{PgConfig}, Ref{Ptr{Cvoid}}), Ref(cfg), h)
    rc == 0 || error("pg_create failed ($rc): " * unsafe_string(ccall(Libdl.dlsym(L, :pg_last_error), Cstring, (Ptr{Cvoid},), C_NULL)))
    mpc = BatchedTrajectoryTrackingMPC(L, h[], B, zeros(BicycleState{Float64}, B), zeros(BicycleControl{Float64}, B),
                                       zeros(SimpleCarState{Float64}, B), fill(NaN, B), zeros(B))
    finalizer(m -> ccall(Libdl.dlsym(m.lib, :pg_destroy), Cint, (Ptr{Cvoid},), m.handle), mpc)
    set_trajectory!(mpc, trajectory)
    mpc
end
_vehicle(v::Dict{Symbol,Float64}) = PgVehicle((v[k] for k in (:G, :m, :Izz, :L, :a, :b, :h, :μ, :Cαf, :Cαr, :Cd0, :Cd1, :Cd2, :fwd_frac, :rwd_frac, :fwb_frac, :rwb_frac,
                                                               :Fx_max, :Fx_min, :Px_max, :δ_max, :κ_max))...)

"CoupledTrajectoryTrackingMPC(vehicle, trajectory; ...) for a batch of B (src/coupled_lat_long.jl:42-60)"
function BatchedTrajectoryTrackingMPC(vehicle::Dict{Symbol,Float64}, trajectory::TrajectoryTube{Float64}, B::Integer;
                                      control_params=CoupledControlParams(), N_short=10, N_long=20, dt_short=0.01, dt_long=0.2,
                                      use_correction_step=true, device=0, precision::Symbol=:f64, polish=nothing, warm_polish=nothing, cold_guess=nothing)
    L = lib(precision)
    cfg = Ref{PgConfig}()
    ccall(Libdl.dlsym(L, :pg_default_config), Cint, (Ref{PgConfig},), cfg)          # solver tolerances default to the library's own (they depend on its arithmetic type)
    c = cfg[]
    U = control_params
    cp = PgControlParams(U.V_min, U.V_max, U.k_V, U.k_s, U.δ̇_max, U.Q_Δs, U.Q_Δψ, U.Q_e, U.W_β, U.W_r, U.W_HJI, U.R_δ, U.R_Δδ, U.R_Fx, U.R_ΔFx, U.N_HJI, 0)
    _create(PgConfig(_vehicle(vehicle), cp, N_short, N_long, dt_short, dt_long, use_correction_step, c.rk4_substeps, c.hji_eps, B, device,
                     c.ipm_max_iter, 0, c.ipm_tol, c.ipm_mu0, 0, 0, c.wall_weight, polish === nothing ? c.polish : Int32(polish), 0, c.polish_rho, c.polish_tol, c.polish_ipm_tol,
                     warm_polish === nothing ? c.warm_polish : Int32(warm_polish), cold_guess === nothing ? c.cold_guess : Int32(cold_guess)), L, trajectory, B)
end

"DecoupledTrajectoryTrackingMPC(vehicle, trajectory; ...) for a batch of B (src/decoupled_lat_long.jl:32-50).  `walls = true` adds the build-defined soft corridor rows
edge_R - sw <= e <= edge_L + sw from the tube's edge channels (the reference snapshot carries the edges but no constraint reads them, README.md:54)."
function BatchedDecoupledTrajectoryTrackingMPC(vehicle::Dict{Symbol,Float64}, trajectory::TrajectoryTube{Float64}, B::Integer;
                                               control_params=Pigeon.DecoupledControlParams(), N_short=10, N_long=20, dt_short=0.01, dt_long=0.2,
                                               use_correction_step=true, device=0, precision::Symbol=:f64, walls=false, wall_weight=1000.0, polish=nothing, warm_polish=nothing,
                                               allow_f32_long_lateral=false)
    L = lib(precision)
    cfg = Ref{PgConfig}()
    ccall(Libdl.dlsym(L, :pg_default_config_decoupled), Cint, (Ref{PgConfig},), cfg)
    c = cfg[]; d = c.control
    U = control_params                                # the lateral formulation has no Q_Δs / R_Fx / R_ΔFx / W_HJI / N_HJI: those slots keep the library's defaults
    cp = PgControlParams(U.V_min, U.V_max, U.k_V, U.k_s, U.δ̇_max, d.Q_ds, U.Q_Δψ, U.Q_e, U.W_β, U.W_r, d.W_HJI, U.R_δ, U.R_Δδ, d.R_Fx, d.R_dFx, d.N_HJI, 0)
    _create(PgConfig(_vehicle(vehicle), cp, N_short, N_long, dt_short, dt_long, use_correction_step, c.rk4_substeps, c.hji_eps, B, device,
                     c.ipm_max_iter, 1, c.ipm_tol, c.ipm_mu0, walls, Int32(allow_f32_long_lateral), wall_weight, polish === nothing ? c.polish : Int32(polish), 0, c.polish_rho, c.polish_tol, c.polish_ipm_tol,
                     warm_polish === nothing ? c.warm_polish : Int32(warm_polish), c.cold_guess), L, trajectory, B)
end

"mpc.trajectory = latest_trajectory[] (src/ros_integration.jl:53)"
function set_trajectory!(mpc::BatchedTrajectoryTrackingMPC, tj::TrajectoryTube{Float64})
    check(mpc, ccall(sym(mpc, :pg_set_trajectory), Cint, (Ptr{Cvoid}, Int32, ntuple(_ -> Ptr{Float64}, 12)...),
                            mpc.handle, length(tj), tj.t, tj.s, tj.V, tj.A, tj.E, tj.N, tj.ψ, tj.κ, tj.θ, tj.ϕ, tj.edge_L, tj.edge_R), "pg_set_trajectory")
end

"One controller per (x0, reference trajectory) pair: a library of tubes and the tube each instance tracks (0-based index)"
function set_trajectories!(mpc::BatchedTrajectoryTrackingMPC, tubes::Vector{TrajectoryTube{Float64}}, index::Vector{Int32})
    Lmax = maximum(length, tubes); L = Int32[length(t) for t in tubes]
    pack = zeros(Float64, Lmax, 10, length(tubes))                       # column-major [L][channel][tube] == the ABI's [n_traj][10][Lmax]
    for (k, t) in enumerate(tubes), (c, ch) in enumerate((t.t, t.s, t.V, t.A, t.E, t.N, t.ψ, t.κ, t.edge_L, t.edge_R))
        pack[1:length(t), c, k] .= ch
    end
    check(mpc, ccall(sym(mpc, :pg_set_trajectories), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Float64}), mpc.handle, length(tubes), Lmax, L, pack), "pg_set_trajectories")
    check(mpc, ccall(sym(mpc, :pg_set_trajectory_index), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}), mpc.handle, length(index), index), "pg_set_trajectory_index")
end

"One controller per (x0, control_params) pair (src/coupled_lat_long.jl:42-60, src/decoupled_lat_long.jl:32-50): a library of parameter sets in the ABI's layout and the set each instance runs under (0-based index; may be empty for a library of one)"
function set_control_params!(mpc::BatchedTrajectoryTrackingMPC, sets::Vector{PgControlParams}, index::Vector{Int32}=Int32[])
    check(mpc, ccall(sym(mpc, :pg_set_control_param_sets), Cint, (Ptr{Cvoid}, Int32, Ptr{PgControlParams}), mpc.handle, length(sets), sets), "pg_set_control_param_sets")
    isempty(index) || set_control_param_index!(mpc, index)
end
set_control_param_index!(mpc::BatchedTrajectoryTrackingMPC, index::Vector{Int32}) =
    check(mpc, ccall(sym(mpc, :pg_set_control_param_index), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}), mpc.handle, length(index), index), "pg_set_control_param_index")
"back to the control_params the controller was constructed with"
clear_control_params!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_clear_control_param_sets), Cint, (Ptr{Cvoid},), mpc.handle), "pg_clear_control_param_sets")
"(sets, index over the first B instances; -1 where no index covers an instance) as installed"
function control_param_sets(mpc::BatchedTrajectoryTrackingMPC, B::Integer)
    n = Ref{Int32}(0)
    check(mpc, ccall(sym(mpc, :pg_get_control_param_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgControlParams}, Int32, Ptr{Int32}, Int32), mpc.handle, n, C_NULL, 0, C_NULL, 0), "pg_get_control_param_sets")
    sets = Vector{PgControlParams}(undef, n[]); index = fill(Int32(-1), B)
    check(mpc, ccall(sym(mpc, :pg_get_control_param_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgControlParams}, Int32, Ptr{Int32}, Int32), mpc.handle, n, sets, n[], index, B), "pg_get_control_param_sets")
    sets, index
end

# Plant sets and the tracking summary (pg_set_plant_sets ..., pg_get_tracking_state): like everything in this file, NOT EXECUTED in the build container.
"The vehicle the PLANT of a rollout integrates, per instance (src/model_predictive_control.jl:94 only; the controller keeps its own vehicle): a library of vehicles in the ABI's layout (`_vehicle(X1())`) and the set each instance runs under (0-based index; may be empty for a library of one).  Resets nothing."
function set_plants!(mpc::BatchedTrajectoryTrackingMPC, sets::Vector{PgVehicle}, index::Vector{Int32}=Int32[])
    check(mpc, ccall(sym(mpc, :pg_set_plant_sets), Cint, (Ptr{Cvoid}, Int32, Ptr{PgVehicle}), mpc.handle, length(sets), sets), "pg_set_plant_sets")
    isempty(index) || set_plant_index!(mpc, index)
end
set_plant_index!(mpc::BatchedTrajectoryTrackingMPC, index::Vector{Int32}) =
    check(mpc, ccall(sym(mpc, :pg_set_plant_index), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}), mpc.handle, length(index), index), "pg_set_plant_index")
"back to the vehicle the controller was constructed with"
clear_plants!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_clear_plant_sets), Cint, (Ptr{Cvoid},), mpc.handle), "pg_clear_plant_sets")
"(sets, index over the first B instances; -1 where no index covers an instance) as installed"
function plant_sets(mpc::BatchedTrajectoryTrackingMPC, B::Integer)
    n = Ref{Int32}(0)
    check(mpc, ccall(sym(mpc, :pg_get_plant_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgVehicle}, Int32, Ptr{Int32}, Int32), mpc.handle, n, C_NULL, 0, C_NULL, 0), "pg_get_plant_sets")
    sets = Vector{PgVehicle}(undef, n[]); index = fill(Int32(-1), B)
    check(mpc, ccall(sym(mpc, :pg_get_plant_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgVehicle}, Int32, Ptr{Int32}, Int32), mpc.handle, n, sets, n[], index, B), "pg_get_plant_sets")
    sets, index
end
"Tracking summary of the rollouts since the clock last restarted (option \"tracking_summary\" = 1 first): (summary 6 x B = max |e|, sum e^2, max |Uy / Ux|, max |r|, min Ux, last s; steps; first_exit, 0-based step index or -1)"
function tracking_summary(mpc::BatchedTrajectoryTrackingMPC)
    summary = zeros(6, mpc.B); steps = zeros(Int32, mpc.B); first_exit = zeros(Int32, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_tracking_state), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}), mpc.handle, summary, steps, first_exit), "pg_get_tracking_state")
    summary, steps, first_exit
end

# Sensor sets (pg_set_sensor_sets ...): seeded measurement noise in the three rollouts.  NOT EXECUTED in the build container, like the rest of this file.
"One sensor: per channel of (E, N, psi, Ux, Uy, r) a standard deviation and a constant bias (pg_sensor)"
struct PgSensor
    sigma::NTuple{6,Float64}
    bias::NTuple{6,Float64}
end
PgSensor(; sigma=zeros(6), bias=zeros(6)) = PgSensor(Tuple(Float64.(sigma)), Tuple(Float64.(bias)))
"What the CONTROLLER of a rollout step reads in place of the true state: measured = true + bias + sigma z per channel (the plant, the records and the tracking summary keep the truth).  A library of sensors, the set each instance runs under (0-based; may be empty for a library of one), the seed and the 64-bit stream ids of the draws (empty: stream[b] = b).  Resets nothing."
function set_sensors!(mpc::BatchedTrajectoryTrackingMPC, sets::Vector{PgSensor}, index::Vector{Int32}=Int32[]; seed::UInt64=UInt64(0), streams::Vector{UInt64}=UInt64[])
    check(mpc, ccall(sym(mpc, :pg_set_sensor_sets), Cint, (Ptr{Cvoid}, Int32, Ptr{PgSensor}), mpc.handle, length(sets), sets), "pg_set_sensor_sets")
    isempty(index) || check(mpc, ccall(sym(mpc, :pg_set_sensor_index), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}), mpc.handle, length(index), index), "pg_set_sensor_index")
    check(mpc, ccall(sym(mpc, :pg_set_sensor_seed), Cint, (Ptr{Cvoid}, UInt64, Int32, Ptr{UInt64}), mpc.handle, seed, isempty(streams) ? max(mpc.B, 1) : length(streams),
                     isempty(streams) ? C_NULL : streams), "pg_set_sensor_seed")
end
"back to measured = true"
clear_sensors!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_clear_sensor_sets), Cint, (Ptr{Cvoid},), mpc.handle), "pg_clear_sensor_sets")
"(sets, index over the first B instances; -1 where no index covers an instance) as installed"
function sensors(mpc::BatchedTrajectoryTrackingMPC, B::Integer)
    n = Ref{Int32}(0)
    check(mpc, ccall(sym(mpc, :pg_get_sensor_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgSensor}, Int32, Ptr{Int32}, Int32), mpc.handle, n, C_NULL, 0, C_NULL, 0), "pg_get_sensor_sets")
    sets = Vector{PgSensor}(undef, n[]); index = fill(Int32(-1), B)
    check(mpc, ccall(sym(mpc, :pg_get_sensor_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgSensor}, Int32, Ptr{Int32}, Int32), mpc.handle, n, sets, n[], index, B), "pg_get_sensor_sets")
    sets, index
end
"The standard normals the rollouts draw at clock steps step0 .. step0 + steps - 1 (0-based), 6 x B x steps, computed on the device by the function the rollouts call"
function sensor_draws(mpc::BatchedTrajectoryTrackingMPC, step0::Integer, steps::Integer, B::Integer=mpc.B)
    z = zeros(6, B, steps)
    check(mpc, ccall(sym(mpc, :pg_sensor_draws), Cint, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float64}), mpc.handle, step0, steps, B, z), "pg_sensor_draws")
    z
end
"6 x B: what the controller read at the last rollout step under a sensor library"
function measured_state(mpc::BatchedTrajectoryTrackingMPC)
    m = zeros(6, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_measured_state), Cint, (Ptr{Cvoid}, Ptr{Float64}), mpc.handle, m), "pg_get_measured_state")
    m
end
"The NEXT rollout call writes the measured state of its step k < steps to a device array 6 x B x steps of the library's element type (one-shot; C_NULL cancels)"
set_measured_history!(mpc::BatchedTrajectoryTrackingMPC, buf::Ptr{Cvoid}, steps::Integer) =
    check(mpc, ccall(sym(mpc, :pg_set_measured_history_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), mpc.handle, buf, steps), "pg_set_measured_history_dev")

# Actuator sets (pg_set_actuator_sets ...): command delay, lag and slew between the controller and the plant of the rollouts.  NOT EXECUTED in the build container, like the rest of this file.
const PG_ACT_MAX_DELAY = 16
"One actuator (pg_actuator_set): transport delay in rollout steps (0 .. PG_ACT_MAX_DELAY), what the controller sees as current_control (0: the command last sent, src/ros_integration.jl:52; 1: the actuator's position, the commented-out :51), first-order time constants (s; 0 = none) and slew limits (rad/s, N/s; Inf = none) of steering and of each longitudinal force channel.  PgActuatorSet() is the identity: the handle without a library, bit for bit."
struct PgActuatorSet
    delay_steps::Int32
    feedback::Int32
    tau_delta::Float64
    tau_fx::Float64
    rate_delta::Float64
    rate_fx::Float64
end
PgActuatorSet(; delay_steps=0, feedback=0, tau_delta=0.0, tau_fx=0.0, rate_delta=Inf, rate_fx=Inf) = PgActuatorSet(Int32(delay_steps), Int32(feedback), Float64(tau_delta), Float64(tau_fx), Float64(rate_delta), Float64(rate_fx))
"layout self-check of the hand copy above against include/pigeon_mpc.h (two int32, then four doubles: 40 bytes, no padding)"
function check_actuator_layout()
    off(f) = Int(fieldoffset(PgActuatorSet, Base.fieldindex(PgActuatorSet, f)))
    (sizeof(PgActuatorSet), off(:delay_steps), off(:feedback), off(:tau_delta), off(:tau_fx), off(:rate_delta), off(:rate_fx)) == (40, 0, 4, 8, 16, 24, 32) ||
        error("PigeonMI355X.jl: PgActuatorSet differs from pg_actuator_set of include/pigeon_mpc.h")
end
"What the PLANT of simulate / the safety rollout integrates in place of the command: a library of actuators and the set each instance runs under (0-based; may be empty for a library of one).  Resets nothing.  The node rollout refuses to run under a library."
function set_actuators!(mpc::BatchedTrajectoryTrackingMPC, sets::Vector{PgActuatorSet}, index::Vector{Int32}=Int32[])
    check_actuator_layout()
    check(mpc, ccall(sym(mpc, :pg_set_actuator_sets), Cint, (Ptr{Cvoid}, Int32, Ptr{PgActuatorSet}), mpc.handle, length(sets), sets), "pg_set_actuator_sets")
    isempty(index) || check(mpc, ccall(sym(mpc, :pg_set_actuator_index), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}), mpc.handle, length(index), index), "pg_set_actuator_index")
end
"back to applied = command"
clear_actuators!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_clear_actuator_sets), Cint, (Ptr{Cvoid},), mpc.handle), "pg_clear_actuator_sets")
"(sets, index over the first B instances; -1 where no index covers an instance) as installed"
function actuators(mpc::BatchedTrajectoryTrackingMPC, B::Integer)
    n = Ref{Int32}(0)
    check(mpc, ccall(sym(mpc, :pg_get_actuator_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgActuatorSet}, Int32, Ptr{Int32}, Int32), mpc.handle, n, C_NULL, 0, C_NULL, 0), "pg_get_actuator_sets")
    sets = Vector{PgActuatorSet}(undef, n[]); index = fill(Int32(-1), B)
    check(mpc, ccall(sym(mpc, :pg_get_actuator_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgActuatorSet}, Int32, Ptr{Int32}, Int32), mpc.handle, n, sets, n[], index, B), "pg_get_actuator_sets")
    sets, index
end
"3 x B: the applied control of the last rollout step under an actuator library (the handle's control before the first one since the clock restarted)"
function actuator_state(mpc::BatchedTrajectoryTrackingMPC)
    a = zeros(3, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_actuator_state), Cint, (Ptr{Cvoid}, Ptr{Float64}), mpc.handle, a), "pg_get_actuator_state")
    a
end
"The law alone, on the device: commands 3 x B x steps -> applied 3 x B x steps under the installed library and index, from a fresh state"
function actuator_response(mpc::BatchedTrajectoryTrackingMPC, commands::Array{Float64,3}, dt::Float64)
    applied = similar(commands)
    check(mpc, ccall(sym(mpc, :pg_actuator_response), Cint, (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}, Ptr{Float64}), mpc.handle, size(commands, 3), dt, commands, applied), "pg_actuator_response")
    applied
end
"The NEXT rollout call writes the applied control / the command of its step k < steps to a device array 3 x B x steps of the library's element type (one-shot; C_NULL cancels)"
set_applied_history!(mpc::BatchedTrajectoryTrackingMPC, buf::Ptr{Cvoid}, steps::Integer) =
    check(mpc, ccall(sym(mpc, :pg_set_applied_history_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), mpc.handle, buf, steps), "pg_set_applied_history_dev")
set_command_history!(mpc::BatchedTrajectoryTrackingMPC, buf::Ptr{Cvoid}, steps::Integer) =
    check(mpc, ccall(sym(mpc, :pg_set_command_history_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), mpc.handle, buf, steps), "pg_set_command_history_dev")

# Disturbance sets (pg_set_disturbance_sets ...): forces, a seeded gust and low-friction windows on the ego plant of the rollouts.  NOT EXECUTED in the build container, like the rest of this file.

"One disturbance (pg_disturbance): the window in clock steps (step_on <= k, and k < step_off unless step_off < 0), the constant body-frame force (N) and yaw moment (N m), the gust's standard deviations (N), the lever arm of its side force (m), its correlation time (s; 0 = white) and the factor on the plant's mu while active.  PgDisturbance() is the identity: the handle without a library, bit for bit."
struct PgDisturbance
    step_on::Int32
    step_off::Int32
    Fx::Float64
    Fy::Float64
    Mz::Float64
    sigma_Fx::Float64
    sigma_Fy::Float64
    x_cp::Float64
    tau_gust::Float64
    mu_scale::Float64
end
PgDisturbance(; step_on=0, step_off=-1, Fx=0.0, Fy=0.0, Mz=0.0, sigma_Fx=0.0, sigma_Fy=0.0, x_cp=0.0, tau_gust=0.0, mu_scale=1.0) =
    PgDisturbance(Int32(step_on), Int32(step_off), Float64(Fx), Float64(Fy), Float64(Mz), Float64(sigma_Fx), Float64(sigma_Fy), Float64(x_cp), Float64(tau_gust), Float64(mu_scale))
"the layout include/pigeon_mpc.h states (72 bytes): checked before the first install"
function check_disturbance_layout()
    off(f) = Int(fieldoffset(PgDisturbance, Base.fieldindex(PgDisturbance, f)))
    (sizeof(PgDisturbance), off(:step_on), off(:step_off), off(:Fx), off(:Fy), off(:Mz), off(:sigma_Fx), off(:sigma_Fy), off(:x_cp), off(:tau_gust), off(:mu_scale)) ==
        (72, 0, 4, 8, 16, 24, 32, 40, 48, 56, 64) || error("PigeonMI355X.jl: PgDisturbance differs from pg_disturbance of include/pigeon_mpc.h")
end
"What acts on the ego PLANT of the three rollouts from outside: a library of disturbances and the set each instance runs under (0-based; may be empty for a library of one).  The controller never sees it.  Resets nothing."
function set_disturbances!(mpc::BatchedTrajectoryTrackingMPC, sets::Vector{PgDisturbance}, index::Vector{Int32}=Int32[])
    check_disturbance_layout()
    check(mpc, ccall(sym(mpc, :pg_set_disturbance_sets), Cint, (Ptr{Cvoid}, Int32, Ptr{PgDisturbance}), mpc.handle, length(sets), sets), "pg_set_disturbance_sets")
    isempty(index) || check(mpc, ccall(sym(mpc, :pg_set_disturbance_index), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}), mpc.handle, length(index), index), "pg_set_disturbance_index")
    nothing
end
"Key of the gust's draws and the 64-bit stream id of every instance (empty: stream[b] = b); both persist across a clear"
function set_disturbance_seed!(mpc::BatchedTrajectoryTrackingMPC, seed::UInt64, streams::Vector{UInt64}=UInt64[])
    check(mpc, ccall(sym(mpc, :pg_set_disturbance_seed), Cint, (Ptr{Cvoid}, UInt64, Int32, Ptr{UInt64}), mpc.handle, seed, isempty(streams) ? mpc.B : length(streams),
                     isempty(streams) ? C_NULL : pointer(streams)), "pg_set_disturbance_seed")
end
clear_disturbances!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_clear_disturbance_sets), Cint, (Ptr{Cvoid},), mpc.handle), "pg_clear_disturbance_sets")
"(sets, index over B instances; -1 where no index covers an instance) as installed"
function disturbances(mpc::BatchedTrajectoryTrackingMPC, B::Integer)
    n = Ref{Int32}(0)
    check(mpc, ccall(sym(mpc, :pg_get_disturbance_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgDisturbance}, Int32, Ptr{Int32}, Int32), mpc.handle, n, C_NULL, 0, C_NULL, 0), "pg_get_disturbance_sets")
    sets = Vector{PgDisturbance}(undef, n[]); index = fill(Int32(-1), B)
    check(mpc, ccall(sym(mpc, :pg_get_disturbance_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgDisturbance}, Int32, Ptr{Int32}, Int32), mpc.handle, n, sets, n[], index, B), "pg_get_disturbance_sets")
    sets, index
end
"The law alone, on the device: w 4 x B x steps = (wFx, wFy, wMz, wmu) of the clock steps step0 .. step0 + steps - 1 under the installed library, index, seed and streams, from a fresh gust state"
function disturbance_response(mpc::BatchedTrajectoryTrackingMPC, step0::Integer, steps::Integer, dt::Float64)
    w = zeros(4, mpc.B, steps)
    check(mpc, ccall(sym(mpc, :pg_disturbance_response), Cint, (Ptr{Cvoid}, Int32, Int32, Float64, Ptr{Float64}), mpc.handle, step0, steps, dt, w), "pg_disturbance_response")
    w
end
"4 x B: w of the last rollout step under a disturbance library"
function disturbance_state(mpc::BatchedTrajectoryTrackingMPC)
    w = zeros(4, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_disturbance_state), Cint, (Ptr{Cvoid}, Ptr{Float64}), mpc.handle, w), "pg_get_disturbance_state")
    w
end
"The NEXT rollout call writes w of its step k < steps to a device array 4 x B x steps of the library's element type (one-shot; C_NULL cancels)"
set_disturbance_history!(mpc::BatchedTrajectoryTrackingMPC, buf::Ptr{Cvoid}, steps::Integer) =
    check(mpc, ccall(sym(mpc, :pg_set_disturbance_history_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), mpc.handle, buf, steps), "pg_set_disturbance_history_dev")

# Estimator sets (pg_set_estimator_sets ...): a fixed-gain observer between the sensor and the controller of the rollouts.  NOT EXECUTED in the build container, like the rest of this file.

"One estimator (pg_estimator): predict = 1 takes one step of the controller's own model from the previous estimate as the prior, predict = 0 the previous estimate itself; reserved is 0; gain per channel of (E, N, psi, Ux, Uy, r) in [0, 1], estimate = prior + gain (measurement - prior).  PgEstimator() is the identity (every gain 1): the handle without a library, bit for bit."
struct PgEstimator
    predict::Int32
    reserved::Int32
    gain::NTuple{6,Float64}
end
PgEstimator(; predict=1, gain=ntuple(_ -> 1.0, 6)) = PgEstimator(Int32(predict), Int32(0), gain isa Real ? ntuple(_ -> Float64(gain), 6) : NTuple{6,Float64}(Float64.(Tuple(gain))))
"the layout include/pigeon_mpc.h states (56 bytes): checked before the first install"
function check_estimator_layout()
    off(f) = Int(fieldoffset(PgEstimator, Base.fieldindex(PgEstimator, f)))
    (sizeof(PgEstimator), off(:predict), off(:reserved), off(:gain)) == (56, 0, 4, 8) || error("PigeonMI355X.jl: PgEstimator differs from pg_estimator of include/pigeon_mpc.h")
end
"What the CONTROLLER of the three rollouts reads in place of the sensor's output: a library of estimators and the set each instance runs under (0-based; may be empty for a library of one).  The plant, the records and the summaries keep the truth.  Resets nothing."
function set_estimators!(mpc::BatchedTrajectoryTrackingMPC, sets::Vector{PgEstimator}, index::Vector{Int32}=Int32[])
    check_estimator_layout()
    check(mpc, ccall(sym(mpc, :pg_set_estimator_sets), Cint, (Ptr{Cvoid}, Int32, Ptr{PgEstimator}), mpc.handle, length(sets), sets), "pg_set_estimator_sets")
    isempty(index) || check(mpc, ccall(sym(mpc, :pg_set_estimator_index), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}), mpc.handle, length(index), index), "pg_set_estimator_index")
    nothing
end
clear_estimators!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_clear_estimator_sets), Cint, (Ptr{Cvoid},), mpc.handle), "pg_clear_estimator_sets")
"(sets, index over B instances; -1 where no index covers an instance) as installed"
function get_estimators(mpc::BatchedTrajectoryTrackingMPC, B::Integer)
    n = Ref{Int32}(0)
    check(mpc, ccall(sym(mpc, :pg_get_estimator_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgEstimator}, Int32, Ptr{Int32}, Int32), mpc.handle, n, C_NULL, 0, C_NULL, 0), "pg_get_estimator_sets")
    sets = Vector{PgEstimator}(undef, n[]); index = fill(Int32(-1), B)
    check(mpc, ccall(sym(mpc, :pg_get_estimator_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgEstimator}, Int32, Ptr{Int32}, Int32), mpc.handle, n, sets, n[], index, B), "pg_get_estimator_sets")
    sets, index
end
"6 x B: the estimate the controller read at the last rollout step under an estimator library"
function estimated_state(mpc::BatchedTrajectoryTrackingMPC)
    e = zeros(6, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_estimated_state), Cint, (Ptr{Cvoid}, Ptr{Float64}), mpc.handle, e), "pg_get_estimated_state")
    e
end
"The NEXT rollout call writes the estimate of its step k < steps to a device array 6 x B x steps of the library's element type (one-shot; C_NULL cancels)"
set_estimated_history!(mpc::BatchedTrajectoryTrackingMPC, buf::Ptr{Cvoid}, steps::Integer) =
    check(mpc, ccall(sym(mpc, :pg_set_estimated_history_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), mpc.handle, buf, steps), "pg_set_estimated_history_dev")
"The law alone, on the device: measurements y 6 x B x steps and controls u 3 x B x steps (u[:, :, k]: what the controller is handed at step k) -> estimates 6 x B x steps under the installed library and index, from a fresh state"
function estimator_response(mpc::BatchedTrajectoryTrackingMPC, y::Array{Float64,3}, u::Array{Float64,3}, dt::Float64)
    xhat = zeros(size(y))
    check(mpc, ccall(sym(mpc, :pg_estimator_response), Cint, (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), mpc.handle, size(y, 3), dt, y, u, xhat), "pg_estimator_response")
    xhat
end

# Human sets (pg_set_human_sets ...): the driver of the other car in the safety and node rollouts, per instance.  NOT EXECUTED in the build container, like the rest of this file.

"One driver of the other car (pg_human): mode 0 hold, 1 worst case (optimal_disturbance), 2 the caller's script, 3 seeded random; a decision is kept for hold_steps steps, counted from step_on; active at clock steps step_on <= k < step_off (step_off < 0: open-ended); gain on the decided (omega, a) in [0, 1]; |omega| <= omega_max, a_min <= a <= a_max (Inf: no limit); sigma and tau of the random driver.  PgHuman(mode = m) for m in 0:2 is the identity: the rollouts' human_mode = m, bit for bit."
struct PgHuman
    mode::Int32
    hold_steps::Int32
    step_on::Int32
    step_off::Int32
    gain::NTuple{2,Float64}
    omega_max::Float64
    a_min::Float64
    a_max::Float64
    sigma::NTuple{2,Float64}
    tau::Float64
end
PgHuman(; mode=0, hold_steps=1, step_on=0, step_off=-1, gain=(1.0, 1.0), omega_max=Inf, a_min=-Inf, a_max=Inf, sigma=(0.0, 0.0), tau=0.0) =
    PgHuman(Int32(mode), Int32(hold_steps), Int32(step_on), Int32(step_off), gain isa Real ? (Float64(gain), Float64(gain)) : NTuple{2,Float64}(Float64.(Tuple(gain))), Float64(omega_max),
            Float64(a_min), Float64(a_max), sigma isa Real ? (Float64(sigma), Float64(sigma)) : NTuple{2,Float64}(Float64.(Tuple(sigma))), Float64(tau))
"the layout include/pigeon_mpc.h states (80 bytes): checked before the first install"
function check_human_layout()
    off(f) = Int(fieldoffset(PgHuman, Base.fieldindex(PgHuman, f)))
    (sizeof(PgHuman), off(:mode), off(:hold_steps), off(:step_on), off(:step_off), off(:gain), off(:omega_max), off(:a_min), off(:a_max), off(:sigma), off(:tau)) ==
        (80, 0, 4, 8, 12, 16, 32, 40, 48, 56, 72) || error("PigeonMI355X.jl: PgHuman differs from pg_human of include/pigeon_mpc.h")
end
"Who drives the other car of the safety and node rollouts: a library of drivers and the set each instance runs under (0-based; may be empty for a library of one).  Under a library the rollouts' human_mode no longer decides; human_u is wanted when a set has mode 2.  Resets nothing."
function set_humans!(mpc::BatchedTrajectoryTrackingMPC, sets::Vector{PgHuman}, index::Vector{Int32}=Int32[])
    check_human_layout()
    check(mpc, ccall(sym(mpc, :pg_set_human_sets), Cint, (Ptr{Cvoid}, Int32, Ptr{PgHuman}), mpc.handle, length(sets), sets), "pg_set_human_sets")
    isempty(index) || check(mpc, ccall(sym(mpc, :pg_set_human_index), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}), mpc.handle, length(index), index), "pg_set_human_index")
    nothing
end
"key of the random driver's draws and the 64-bit stream id per instance (empty: stream[b] = b - 1)"
set_human_seed!(mpc::BatchedTrajectoryTrackingMPC, seed::UInt64, streams::Vector{UInt64}=UInt64[]) =
    check(mpc, ccall(sym(mpc, :pg_set_human_seed), Cint, (Ptr{Cvoid}, UInt64, Int32, Ptr{UInt64}), mpc.handle, seed, isempty(streams) ? max(mpc.B, 1) : length(streams), isempty(streams) ? C_NULL : pointer(streams)), "pg_set_human_seed")
clear_humans!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_clear_human_sets), Cint, (Ptr{Cvoid},), mpc.handle), "pg_clear_human_sets")
"(sets, index over B instances; -1 where no index covers an instance) as installed"
function humans(mpc::BatchedTrajectoryTrackingMPC, B::Integer)
    n = Ref{Int32}(0)
    check(mpc, ccall(sym(mpc, :pg_get_human_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgHuman}, Int32, Ptr{Int32}, Int32), mpc.handle, n, C_NULL, 0, C_NULL, 0), "pg_get_human_sets")
    sets = Vector{PgHuman}(undef, n[]); index = fill(Int32(-1), B)
    check(mpc, ccall(sym(mpc, :pg_get_human_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgHuman}, Int32, Ptr{Int32}, Int32), mpc.handle, n, sets, n[], index, B), "pg_get_human_sets")
    sets, index
end
"2 x B: (omega, a) of the last rollout step under a human library"
function human_state(mpc::BatchedTrajectoryTrackingMPC)
    u = zeros(2, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_human_state), Cint, (Ptr{Cvoid}, Ptr{Float64}), mpc.handle, u), "pg_get_human_state")
    u
end
"The NEXT rollout call writes (omega, a) of its step k < steps to a device array 2 x B x steps of the library's element type (one-shot; C_NULL cancels)"
set_human_history!(mpc::BatchedTrajectoryTrackingMPC, buf::Ptr{Cvoid}, steps::Integer) =
    check(mpc, ccall(sym(mpc, :pg_set_human_history_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), mpc.handle, buf, steps), "pg_set_human_history_dev")
"The law alone, on the device: relative states x7 7 x B x steps, lookups vg8 8 x B x steps (V, then the gradient) and a script 2 x B x steps (nothing: none) -> (omega, a) 2 x B x steps of the clock steps step0, step0 + 1, ... under the installed library, index, seed and streams, from a fresh state"
function human_response(mpc::BatchedTrajectoryTrackingMPC, step0::Integer, x7::Array{Float64,3}, vg8::Array{Float64,3}, dt::Float64, script::Union{Nothing,Array{Float64,3}}=nothing)
    u = zeros(2, size(x7, 2), size(x7, 3))
    check(mpc, ccall(sym(mpc, :pg_human_response), Cint, (Ptr{Cvoid}, Int32, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), mpc.handle, step0, size(x7, 3), dt, x7, vg8,
                     script === nothing ? C_NULL : pointer(script), u), "pg_human_response")
    u
end

# Route sets (pg_set_route_sets ...): an instance changes trajectory during a rollout (nominal_trajectory_callback).  NOT EXECUTED in the build container, like the rest of this file.

const PG_ROUTE_EVENTS = 4
const ROUTE_ANCHORS = Dict(:keep => Int32(0), :path => Int32(1), :stamp => Int32(2), :project => Int32(3))
"One event of a route set (pg_route_event): at clock step `step` (< 0: unused slot), ahead of that step's controller, go to trajectory `target` of the installed library (0-based; relative = true: `target` trajectories on from the current one, modulo the library), anchored :keep (time_offset stays), :path (NaN), :stamp (the new trajectory's t = t_join is now) or :project (the seen state projected on the target, t_join further on); cold = true sets solved = false as the reference's callback does."
struct PgRouteEvent
    step::Int32
    target::Int32
    target_mode::Int32
    anchor::Int32
    cold::Int32
    reserved::Int32
    t_join::Float64
end
PgRouteEvent(step, target; anchor::Symbol=:stamp, relative::Bool=false, cold::Bool=true, t_join=0.0) =
    PgRouteEvent(Int32(step), Int32(target), Int32(relative), ROUTE_ANCHORS[anchor], Int32(cold), Int32(0), Float64(t_join))
"One route set (pg_route): up to four events in the order of their steps; PgRoute() is the identity (no event)."
struct PgRoute
    ev::NTuple{4,PgRouteEvent}
end
PgRoute(events::PgRouteEvent...) = PgRoute(ntuple(k -> k <= length(events) ? events[k] : PgRouteEvent(-1, 0), PG_ROUTE_EVENTS))
"the layout include/pigeon_mpc.h states (32 and 128 bytes): checked before the first install"
function check_route_layout()
    off(f) = Int(fieldoffset(PgRouteEvent, Base.fieldindex(PgRouteEvent, f)))
    (sizeof(PgRoute), sizeof(PgRouteEvent), off(:step), off(:target), off(:target_mode), off(:anchor), off(:cold), off(:reserved), off(:t_join)) ==
        (128, 32, 0, 4, 8, 12, 16, 20, 24) || error("PigeonMI355X.jl: PgRoute differs from pg_route of include/pigeon_mpc.h")
end
"the identity set as the library makes it"
default_route(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_route), PgRoute, ())
"Which trajectory of the installed library an instance tracks when: a library of route sets and the set each instance runs under (0-based; may be empty for a library of one).  The index set_trajectory_index! installed is every instance's home: a restarted rollout clock starts there again."
function set_routes!(mpc::BatchedTrajectoryTrackingMPC, sets::Vector{PgRoute}, index::Vector{Int32}=Int32[])
    check_route_layout()
    check(mpc, ccall(sym(mpc, :pg_set_route_sets), Cint, (Ptr{Cvoid}, Int32, Ptr{PgRoute}), mpc.handle, length(sets), sets), "pg_set_route_sets")
    isempty(index) || check(mpc, ccall(sym(mpc, :pg_set_route_index), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}), mpc.handle, length(index), index), "pg_set_route_index")
    nothing
end
clear_routes!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_clear_route_sets), Cint, (Ptr{Cvoid},), mpc.handle), "pg_clear_route_sets")
"(sets, index over B instances; -1 where no index covers an instance) as installed"
function routes(mpc::BatchedTrajectoryTrackingMPC, B::Integer)
    n = Ref{Int32}(0)
    check(mpc, ccall(sym(mpc, :pg_get_route_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgRoute}, Int32, Ptr{Int32}, Int32), mpc.handle, n, C_NULL, 0, C_NULL, 0), "pg_get_route_sets")
    sets = Vector{PgRoute}(undef, n[]); index = fill(Int32(-1), B)
    check(mpc, ccall(sym(mpc, :pg_get_route_sets), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{PgRoute}, Int32, Ptr{Int32}, Int32), mpc.handle, n, sets, n[], index, B), "pg_get_route_sets")
    sets, index
end
"(traj (0-based), fired, last_step, t_at, e_at), B each: where every instance is now and what its last event did"
function route_state(mpc::BatchedTrajectoryTrackingMPC)
    traj = zeros(Int32, mpc.B); fired = zeros(Int32, mpc.B); last_step = zeros(Int32, mpc.B); t_at = zeros(mpc.B); e_at = zeros(mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_route_state), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}), mpc.handle, traj, fired, last_step, t_at, e_at), "pg_get_route_state")
    traj, fired, last_step, t_at, e_at
end
"The NEXT rollout call writes the trajectory the controller of its step k < steps ran on to a device array B x steps of Int32 (one-shot; (C_NULL, 0) cancels)"
set_route_history!(mpc::BatchedTrajectoryTrackingMPC, buf::Ptr{Cvoid}, steps::Integer) =
    check(mpc, ccall(sym(mpc, :pg_set_route_history_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), mpc.handle, buf, steps), "pg_set_route_history_dev")

"mpc.HJI_cache = HJICache(fname) (src/Pigeon.jl:40): hand over grid_knots, V_raw, ∇V_raw exactly as stored in the JLD2 file"
function set_hji_cache!(mpc::BatchedTrajectoryTrackingMPC, grid_knots::NTuple{7,Vector{Float32}}, V_raw::Array{Float32,7}, ∇V_raw::Array{Float32})
    dims = Int32[length(k) for k in grid_knots]
    check(mpc, ccall(sym(mpc, :pg_set_hji_grid), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                            mpc.handle, dims, vcat(grid_knots...), V_raw, ∇V_raw), "pg_set_hji_grid")
end

# Making a grid (pg_hji_solve): the avoid set computed on the device.  NOT EXECUTED in the build container, like the rest of this file.
const PG_HJI_PERIODIC_PSI = Int32(1)
"pg_hji_solve_opts (32 bytes): horizon (s), CFL number in (0, 1], a fixed step (0: the CFL rule), the bound on the sweeps, the flags"
struct PgHjiSolveOpts
    horizon::Float64
    cfl::Float64
    fixed_dt::Float64
    max_sweeps::Int32
    flags::Int32
end
PgHjiSolveOpts(; horizon=3.0, cfl=0.8, fixed_dt=0.0, max_sweeps=100000, periodic_psi=false) =
    PgHjiSolveOpts(Float64(horizon), Float64(cfl), Float64(fixed_dt), Int32(max_sweeps), periodic_psi ? PG_HJI_PERIODIC_PSI : Int32(0))
"pg_hji_solve_stats (104 bytes)"
struct PgHjiSolveStats
    sweeps::Int32
    reached_horizon::Int32
    bad_sweep::Int32
    reserved::Int32
    tau::Float64
    last_dt::Float64
    alpha::NTuple{7,Float64}
    v_min::Float64
    v_max::Float64
end
"The reachable tube of the target l0 over opts.horizon for `vehicle` (nothing: the handle's own): (V_raw, ∇V_raw, stats) as set_hji_cache! takes them; install = true leaves the handle as set_hji_cache! would, without a host round trip (stands in for the toolbox run behind deps/build.jl:1-4)"
function solve_hji_cache!(mpc::BatchedTrajectoryTrackingMPC, grid_knots::NTuple{7,Vector{Float32}}, l0::Array{Float32,7}, opts::PgHjiSolveOpts=PgHjiSolveOpts();
                          vehicle::Union{Nothing,PgVehicle}=nothing, install::Bool=true)
    (sizeof(PgHjiSolveOpts), sizeof(PgHjiSolveStats)) == (32, 104) || error("PigeonMI355X.jl: PgHjiSolveOpts / PgHjiSolveStats differ from include/pigeon_mpc.h")
    dims = Int32[length(k) for k in grid_knots]
    V = zeros(Float32, size(l0)); g = zeros(Float32, 7, size(l0)...)
    stats = Ref{PgHjiSolveStats}()
    veh = vehicle === nothing ? Ptr{PgVehicle}(C_NULL) : Ref(vehicle)
    check(mpc, ccall(sym(mpc, :pg_hji_solve), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{PgVehicle}, Ref{PgHjiSolveOpts}, Int32, Ptr{Float32}, Ptr{Float32}, Ref{PgHjiSolveStats}),
                     mpc.handle, dims, vcat(grid_knots...), l0, veh, Ref(opts), Int32(install), V, g, stats), "pg_hji_solve")
    V, g, stats[]
end

"{ horizon 3, cfl 0.8, fixed_dt 0, max_sweeps 100000, flags 0 } as the library states them (pg_default_hji_solve_opts)"
default_hji_solve_opts(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_hji_solve_opts), PgHjiSolveOpts, ())

# Making the speed profile (pg_plan_speeds): friction-limited V, A, t of every (path, plan set) pair on the device.  NOT EXECUTED in the build container, like the rest of this file.
"pg_speed_plan (64 bytes): the share of the friction, the speed cap and floor, the end speeds of an open path (NaN: free), the extra caps on the tangential and lateral acceleration (Inf: none)"
struct PgSpeedPlan
    mu_scale::Float64
    V_max::Float64
    V_floor::Float64
    V_start::Float64
    V_end::Float64
    ax_max::Float64
    ax_min::Float64
    ay_max::Float64
end
PgSpeedPlan(; mu_scale=1.0, V_max=30.0, V_floor=1.0, V_start=NaN, V_end=NaN, ax_max=Inf, ax_min=-Inf, ay_max=Inf) =
    PgSpeedPlan(Float64(mu_scale), Float64(V_max), Float64(V_floor), Float64(V_start), Float64(V_end), Float64(ax_max), Float64(ax_min), Float64(ay_max))
"pg_speed_plan_stats (48 bytes), one per output trajectory"
struct PgSpeedPlanStats
    t_end::Float64
    v_min::Float64
    v_max::Float64
    usage_max::Float64
    n_cap::Int32
    n_accel::Int32
    n_brake::Int32
    reserved::Int32
end
"channels [Lmax, 10, n_path] (column-major: the C layout [n_path][10][Lmax]; t, V, A ignored), L the knot counts, sets the plan sets -> (channels_out [Lmax, 10, n_path * n_sets], stats); output k = path * n_sets + set (0-based).  closed[k]: knot L[k] is knot 1 again; vehicles: nothing (the handle's) or one per set; install = true leaves the handle as pg_set_trajectories with channels_out would"
function plan_speeds!(mpc::BatchedTrajectoryTrackingMPC, channels::Array{Float64,3}, L::Vector{Int32}, sets::Vector{PgSpeedPlan};
                      closed::Union{Nothing,Vector{Int32}}=nothing, vehicles::Union{Nothing,Vector{PgVehicle}}=nothing, install::Bool=false)
    (sizeof(PgSpeedPlan), sizeof(PgSpeedPlanStats)) == (64, 48) || error("PigeonMI355X.jl: PgSpeedPlan / PgSpeedPlanStats differ from include/pigeon_mpc.h")
    Lmax, ten, n_path = size(channels)
    ten == 10 && length(L) == n_path || error("plan_speeds!: channels is [Lmax, 10, n_path], L has n_path entries")
    vehicles === nothing || length(vehicles) == length(sets) || error("plan_speeds!: one vehicle per set")
    n = n_path * length(sets)
    out = zeros(Float64, Lmax, 10, n); stats = Vector{PgSpeedPlanStats}(undef, n)
    check(mpc, ccall(sym(mpc, :pg_plan_speeds), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Int32, Ptr{PgSpeedPlan}, Ptr{PgVehicle}, Int32, Ptr{Float64}, Ptr{PgSpeedPlanStats}),
                     mpc.handle, Int32(n_path), Int32(Lmax), L, closed === nothing ? Ptr{Int32}(C_NULL) : closed, channels, Int32(length(sets)), sets,
                     vehicles === nothing ? Ptr{PgVehicle}(C_NULL) : vehicles, Int32(install), out, stats), "pg_plan_speeds")
    out, stats
end
"{ 1, 30, 1, NaN, NaN, +Inf, -Inf, +Inf } as the library states them (pg_default_speed_plan)"
default_speed_plan(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_speed_plan), PgSpeedPlan, ())

# Making the path (pg_make_paths): a library of paths from line, arc and clothoid segments on the device.  NOT EXECUTED in the build container, like the rest of this file.
"pg_path_segment (64 bytes): length, the curvature at the start and the end (linear in between: line, arc, clothoid), the tube edges at the start and the end, a reserved 0"
struct PgPathSegment
    length::Float64
    kappa0::Float64
    kappa1::Float64
    edge_L0::Float64
    edge_L1::Float64
    edge_R0::Float64
    edge_R1::Float64
    reserved::Float64
end
PgPathSegment(; length=1.0, kappa0=0.0, kappa1=0.0, edge_L0=4.0, edge_L1=4.0, edge_R0=-4.0, edge_R1=-4.0) =
    PgPathSegment(Float64(length), Float64(kappa0), Float64(kappa1), Float64(edge_L0), Float64(edge_L1), Float64(edge_R0), Float64(edge_R1), 0.0)
"pg_path_spec (48 bytes): the pose of knot 0, the constant speed, the path's segments segments[seg0 + 1 : seg0 + n_seg] (seg0 is 0-based, as in C), its knot count, the caller's `closed`"
struct PgPathSpec
    E0::Float64
    N0::Float64
    psi0::Float64
    V_ref::Float64
    seg0::Int32
    n_seg::Int32
    n_knots::Int32
    closed::Int32
end
"pg_path_stats (48 bytes), one per path"
struct PgPathStats
    length::Float64
    turn::Float64
    closure_pos::Float64
    closure_psi::Float64
    kappa_abs_max::Float64
    ds::Float64
end
"specs and segments as pg_make_paths takes them -> (channels_out [Lmax, 10, n_path] (column-major: the C layout [n_path][10][Lmax]), L, closed, stats); install = true leaves the handle as pg_set_trajectories with channels_out would"
function make_paths!(mpc::BatchedTrajectoryTrackingMPC, specs::Vector{PgPathSpec}, segments::Vector{PgPathSegment}; Lmax::Integer=maximum(s.n_knots for s in specs), install::Bool=false)
    (sizeof(PgPathSegment), sizeof(PgPathSpec), sizeof(PgPathStats)) == (64, 48, 48) || error("PigeonMI355X.jl: PgPathSegment / PgPathSpec / PgPathStats differ from include/pigeon_mpc.h")
    n = length(specs)
    out = zeros(Float64, Lmax, 10, n); L = zeros(Int32, n); closed = zeros(Int32, n); stats = Vector{PgPathStats}(undef, n)
    check(mpc, ccall(sym(mpc, :pg_make_paths), Cint, (Ptr{Cvoid}, Int32, Ptr{PgPathSpec}, Int32, Ptr{PgPathSegment}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{PgPathStats}),
                     mpc.handle, Int32(n), specs, Int32(length(segments)), segments, Int32(Lmax), Int32(install), L, closed, out, stats), "pg_make_paths")
    out, L, closed, stats
end
"{ 1, 0, 0, 4, 4, -4, -4, 0 } as the library states them (pg_default_path_segment)"
default_path_segment(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_path_segment), PgPathSegment, ())

# Fitting the path (pg_fit_paths): a library of paths through waypoints on the device.  NOT EXECUTED in the build container, like the rest of this file.
"pg_waypoint (32 bytes): a surveyed point and the tube edges at it"
struct PgWaypoint
    E::Float64
    N::Float64
    edge_L::Float64
    edge_R::Float64
end
PgWaypoint(; E=0.0, N=0.0, edge_L=4.0, edge_R=-4.0) = PgWaypoint(Float64(E), Float64(N), Float64(edge_L), Float64(edge_R))
"pg_fit_spec (24 bytes): the constant speed, the path's waypoints waypoints[wp0 + 1 : wp0 + n_wp] (wp0 is 0-based, as in C), its knot count, closed (periodic; the first point is not repeated)"
struct PgFitSpec
    V_ref::Float64
    wp0::Int32
    n_wp::Int32
    n_knots::Int32
    closed::Int32
end
"pg_fit_stats (80 bytes), one per path: the six fields of pg_path_stats, then the shortest and the longest chord, what the inversion left, a reserved 0"
struct PgFitStats
    length::Float64
    turn::Float64
    closure_pos::Float64
    closure_psi::Float64
    kappa_abs_max::Float64
    ds::Float64
    chord_min::Float64
    chord_max::Float64
    s_err_max::Float64
    reserved::Float64
end
"specs and waypoints as pg_fit_paths takes them -> (channels_out [Lmax, 10, n_path] (column-major: the C layout [n_path][10][Lmax]), L, closed, stats); install = true leaves the handle as pg_set_trajectories with channels_out would"
function fit_paths!(mpc::BatchedTrajectoryTrackingMPC, specs::Vector{PgFitSpec}, waypoints::Vector{PgWaypoint}; Lmax::Integer=maximum(s.n_knots for s in specs), install::Bool=false)
    (sizeof(PgWaypoint), sizeof(PgFitSpec), sizeof(PgFitStats)) == (32, 24, 80) || error("PigeonMI355X.jl: PgWaypoint / PgFitSpec / PgFitStats differ from include/pigeon_mpc.h")
    n = length(specs)
    out = zeros(Float64, Lmax, 10, n); L = zeros(Int32, n); closed = zeros(Int32, n); stats = Vector{PgFitStats}(undef, n)
    check(mpc, ccall(sym(mpc, :pg_fit_paths), Cint, (Ptr{Cvoid}, Int32, Ptr{PgFitSpec}, Int32, Ptr{PgWaypoint}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{PgFitStats}),
                     mpc.handle, Int32(n), specs, Int32(length(waypoints)), waypoints, Int32(Lmax), Int32(install), L, closed, out, stats), "pg_fit_paths")
    out, L, closed, stats
end
"{ 0, 0, 4, -4 } as the library states them (pg_default_waypoint)"
default_waypoint(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_waypoint), PgWaypoint, ())

# Offsetting the path (pg_offset_paths): lanes, lane changes and pass-bys of a path library on the device.  NOT EXECUTED in the build container, like the rest of this file.
"pg_offset_set (64 bytes): the offset outside the windows and on the plateau, the rise [s_a, s_b] and the fall [s_c, s_d] in the source's arc length (a start of Inf: none), x_min, edge_mode (0 the same road, 1 the tube travels with the path), a reserved 0"
struct PgOffsetSet
    d0::Float64
    d1::Float64
    s_a::Float64
    s_b::Float64
    s_c::Float64
    s_d::Float64
    x_min::Float64
    edge_mode::Int32
    reserved::Int32
end
PgOffsetSet(; d0=0.0, d1=0.0, s_a=Inf, s_b=Inf, s_c=Inf, s_d=Inf, x_min=0.1, edge_mode=0) =
    PgOffsetSet(Float64(d0), Float64(d1), Float64(s_a), Float64(s_b), Float64(s_c), Float64(s_d), Float64(x_min), Int32(edge_mode), Int32(0))
lane(d; kw...) = PgOffsetSet(; d0=d, d1=d, kw...)
lane_change(d0, d1, s_a, s_b; kw...) = PgOffsetSet(; d0=d0, d1=d1, s_a=s_a, s_b=s_b, kw...)
pass_by(d, s_a, s_b, s_c, s_d; kw...) = PgOffsetSet(; d1=d, s_a=s_a, s_b=s_b, s_c=s_c, s_d=s_d, kw...)
"pg_offset_stats (64 bytes), one per output trajectory"
struct PgOffsetStats
    length::Float64
    ds_min::Float64
    ds_max::Float64
    kappa_abs_max::Float64
    x_min::Float64
    d_abs_max::Float64
    closure_pos::Float64
    n_outside::Int32
    reserved::Int32
end
"channels_in [Lmax, 10, n_path] (column-major: the C layout [n_path][10][Lmax]), L and closed as plan_speeds! takes them -> (channels_out [Lmax, 10, n_path * n_sets], L_out, closed_out, stats), trajectory k = path * n_sets + set (0-based); install = true leaves the handle as pg_set_trajectories with channels_out would"
function offset_paths!(mpc::BatchedTrajectoryTrackingMPC, channels_in::Array{Float64,3}, L::Vector{Int32}, closed::Vector{Int32}, sets::Vector{PgOffsetSet}; install::Bool=false)
    (sizeof(PgOffsetSet), sizeof(PgOffsetStats)) == (64, 64) || error("PigeonMI355X.jl: PgOffsetSet / PgOffsetStats differ from include/pigeon_mpc.h")
    Lmax, _, n_path = size(channels_in)
    n = n_path * length(sets)
    out = zeros(Float64, Lmax, 10, n); L_out = zeros(Int32, n); closed_out = zeros(Int32, n); stats = Vector{PgOffsetStats}(undef, n)
    check(mpc, ccall(sym(mpc, :pg_offset_paths), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Int32, Ptr{PgOffsetSet}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{PgOffsetStats}),
                     mpc.handle, Int32(n_path), Int32(Lmax), L, closed, channels_in, Int32(length(sets)), sets, Int32(install), L_out, closed_out, out, stats), "pg_offset_paths")
    out, L_out, closed_out, stats
end
"{ 0, 0, Inf, Inf, Inf, Inf, 0.1, 0, 0 } as the library states them (pg_default_offset_set): the identity"
default_offset_set(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_offset_set), PgOffsetSet, ())

# Clipping the tube (pg_clip_tubes): the tubes of a path library narrowed around obstacle sets on the device.  NOT EXECUTED in the build container, like the rest of this file.
"pg_obstacle (32 bytes): a disc in the world frame, a reserved 0"
struct PgObstacle
    E::Float64
    N::Float64
    radius::Float64
    reserved::Float64
end
PgObstacle(E, N, radius) = PgObstacle(Float64(E), Float64(N), Float64(radius), 0.0)
"pg_obstacle_set (64 bytes): obstacles[first+1 : first+count] of the call's array (first is 0-based, as in C), the margin added to every radius, the taper (Inf: none), the width below which a knot counts as blocked, the side policy (0 centre, 1 wider, 2 pass left, 3 pass right), zeros"
struct PgObstacleSet
    first::Int32
    count::Int32
    margin::Float64
    taper::Float64
    min_width::Float64
    policy::Int32
    reserved::Int32
    pad::NTuple{3,Float64}
end
PgObstacleSet(; first=0, count=0, margin=0.0, taper=Inf, min_width=0.0, policy=0) =
    PgObstacleSet(Int32(first), Int32(count), Float64(margin), Float64(taper), Float64(min_width), Int32(policy), Int32(0), (0.0, 0.0, 0.0))
"pg_clip_stats (64 bytes), one per output trajectory"
struct PgClipStats
    width_min::Float64
    u_width_min::Float64
    reserved_d::NTuple{2,Float64}
    n_clip_L::Int32
    n_clip_R::Int32
    n_blocked::Int32
    n_centre_out::Int32
    n_seen::Int32
    n_ignored::Int32
    reserved::NTuple{2,Int32}
end
"pg_obstacle_report (64 bytes), one per (output trajectory, obstacle slot); the knot indices are 0-based, as in C"
struct PgObstacleReport
    u_at::Float64
    a_at::Float64
    h_at::Float64
    dist_at::Float64
    free_left::Float64
    free_right::Float64
    k_at::Int32
    k_first::Int32
    k_last::Int32
    side::Int32
end
"channels_in [Lmax, 10, n_path], L and closed as offset_paths! takes them -> (channels_out [Lmax, 10, n_path * n_sets], L_out, closed_out, stats, report [max_count, n_path * n_sets]), trajectory k = path * n_sets + set (0-based); install = true leaves the handle as pg_set_trajectories with channels_out would"
function clip_tubes!(mpc::BatchedTrajectoryTrackingMPC, channels_in::Array{Float64,3}, L::Vector{Int32}, closed::Vector{Int32}, sets::Vector{PgObstacleSet}, obstacles::Vector{PgObstacle}; install::Bool=false)
    (sizeof(PgObstacle), sizeof(PgObstacleSet), sizeof(PgClipStats), sizeof(PgObstacleReport)) == (32, 64, 64, 64) || error("PigeonMI355X.jl: the pg_clip_tubes structures differ from include/pigeon_mpc.h")
    Lmax, _, n_path = size(channels_in)
    n = n_path * length(sets)
    max_count = maximum(Int(s.count) for s in sets)
    out = zeros(Float64, Lmax, 10, n); L_out = zeros(Int32, n); closed_out = zeros(Int32, n); stats = Vector{PgClipStats}(undef, n); report = Matrix{PgObstacleReport}(undef, max_count, n)
    check(mpc, ccall(sym(mpc, :pg_clip_tubes), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Int32, Ptr{PgObstacleSet}, Int32, Ptr{PgObstacle}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{PgClipStats}, Ptr{PgObstacleReport}),
                     mpc.handle, Int32(n_path), Int32(Lmax), L, closed, channels_in, Int32(length(sets)), sets, Int32(length(obstacles)), obstacles, Int32(install), L_out, closed_out, out, stats, report), "pg_clip_tubes")
    out, L_out, closed_out, stats, report
end
"{ 0, 0, 0.0, Inf, 0.0, 0, 0, (0, 0, 0) } as the library states them (pg_default_obstacle_set): the identity"
default_obstacle_set(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_obstacle_set), PgObstacleSet, ())

# Refining the path (pg_refine_paths): knots inserted into a path library where a manoeuvre or an obstacle needs them, on the device.  NOT EXECUTED in the build container, like the rest of this file.
"pg_refine_set (128 bytes): the largest spacing wanted everywhere (Inf: none), up to four windows in the source's arc length (s_lo = Inf: unused) with the largest spacing wanted inside each, three reserved zeros"
struct PgRefineSet
    ds::Float64
    s_lo::NTuple{4,Float64}
    s_hi::NTuple{4,Float64}
    ds_w::NTuple{4,Float64}
    reserved::NTuple{3,Float64}
end
"windows: up to four (s_lo, s_hi, ds_w); PgRefineSet() is the identity"
function PgRefineSet(; ds=Inf, windows=())
    length(windows) <= 4 || error("PgRefineSet: at most 4 windows")
    slot(f) = ntuple(j -> j <= length(windows) ? Float64(windows[j][f]) : Inf, 4)
    PgRefineSet(Float64(ds), slot(1), slot(2), slot(3), (0.0, 0.0, 0.0))
end
"pg_refine_stats (64 bytes), one per output trajectory"
struct PgRefineStats
    length::Float64
    ds_min::Float64
    ds_max::Float64
    closure_pos_max::Float64
    closure_psi_max::Float64
    kappa_abs_max::Float64
    n_added::Int32
    m_max::Int32
    reserved::Float64
end
"channels_in [Lmax, 10, n_path], L and closed as offset_paths! takes them, Lmax_out the knot capacity of the output (the library refuses a pair that needs more, naming its count) -> (channels_out [Lmax_out, 10, n_path * n_sets], L_out, closed_out, stats), trajectory k = path * n_sets + set (0-based); install = true leaves the handle as pg_set_trajectories with channels_out would"
function refine_paths!(mpc::BatchedTrajectoryTrackingMPC, channels_in::Array{Float64,3}, L::Vector{Int32}, closed::Vector{Int32}, sets::Vector{PgRefineSet}, Lmax_out::Integer; install::Bool=false)
    (sizeof(PgRefineSet), sizeof(PgRefineStats)) == (128, 64) || error("PigeonMI355X.jl: the pg_refine_paths structures differ from include/pigeon_mpc.h")
    Lmax, _, n_path = size(channels_in)
    n = n_path * length(sets)
    out = zeros(Float64, Lmax_out, 10, n); L_out = zeros(Int32, n); closed_out = zeros(Int32, n); stats = Vector{PgRefineStats}(undef, n)
    check(mpc, ccall(sym(mpc, :pg_refine_paths), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Int32, Ptr{PgRefineSet}, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{PgRefineStats}),
                     mpc.handle, Int32(n_path), Int32(Lmax), L, closed, channels_in, Int32(length(sets)), sets, Int32(Lmax_out), Int32(install), L_out, closed_out, out, stats), "pg_refine_paths")
    out, L_out, closed_out, stats
end
"{ Inf, (Inf x 4), (Inf x 4), (Inf x 4), (0, 0, 0) } as the library states them (pg_default_refine_set): the identity"
default_refine_set(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_refine_set), PgRefineSet, ())

# Smoothing surveyed waypoints (pg_smooth_waypoints): a cubic smoothing spline of every (path, smoothing set) pair, on the device.  NOT EXECUTED in the build container, like the rest of this file.
"pg_smooth_set (120 bytes): lambda in m^3, up to four windows (u_lo, u_hi, factor) in the path's cumulative chord length, of which the first n_win are looked at, the flags pin_ends and keep_walls, a reserved 0"
struct PgSmoothSet
    lambda::Float64
    u_lo::NTuple{4,Float64}
    u_hi::NTuple{4,Float64}
    factor::NTuple{4,Float64}
    n_win::Int32
    pin_ends::Int32
    keep_walls::Int32
    reserved::Int32
end
"windows: up to four (u_lo, u_hi, factor); PgSmoothSet() is the identity"
function PgSmoothSet(; lambda=0.0, windows=(), pin_ends=false, keep_walls=false)
    length(windows) <= 4 || error("PgSmoothSet: at most 4 windows")
    slot(f, fill) = ntuple(j -> j <= length(windows) ? Float64(windows[j][f]) : fill, 4)
    PgSmoothSet(Float64(lambda), slot(1, 0.0), slot(2, 0.0), slot(3, 1.0), Int32(length(windows)), Int32(pin_ends), Int32(keep_walls), Int32(0))
end
"pg_smooth_stats (72 bytes), one per (path, set) pair"
struct PgSmoothStats
    dev_max::Float64
    dev_rms::Float64
    i_dev_max::Float64
    bend::Float64
    n_outside::Float64
    width_min::Float64
    pivot_min::Float64
    chord_min::Float64
    reserved::Float64
end
"specs and waypoints as fit_paths! takes them (only wp0, n_wp and closed are read; the ranges of two paths must not overlap) -> (waypoints_out [n_wp_total, n_sets], stats [n_sets, n_path]): column k is the whole waypoint array under set k, so set k is fitted by adding (k - 1) * n_wp_total to every wp0"
function smooth_waypoints!(mpc::BatchedTrajectoryTrackingMPC, specs::Vector{PgFitSpec}, waypoints::Vector{PgWaypoint}, sets::Vector{PgSmoothSet})
    (sizeof(PgSmoothSet), sizeof(PgSmoothStats)) == (120, 72) || error("PigeonMI355X.jl: the pg_smooth_waypoints structures differ from include/pigeon_mpc.h")
    n, ns, nw = length(specs), length(sets), length(waypoints)
    out = Matrix{PgWaypoint}(undef, nw, ns); stats = Matrix{PgSmoothStats}(undef, ns, n)
    check(mpc, ccall(sym(mpc, :pg_smooth_waypoints), Cint, (Ptr{Cvoid}, Int32, Ptr{PgFitSpec}, Int32, Ptr{PgWaypoint}, Int32, Ptr{PgSmoothSet}, Ptr{PgWaypoint}, Ptr{PgSmoothStats}),
                     mpc.handle, Int32(n), specs, Int32(nw), waypoints, Int32(ns), sets, out, stats), "pg_smooth_waypoints")
    out, stats
end
"{ 0, (0 x 4), (0 x 4), (1 x 4), 0, 0, 0, 0 } as the library states them (pg_default_smooth_set): the identity"
default_smooth_set(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_smooth_set), PgSmoothSet, ())

# Choosing the smoothing weight (pg_tune_smoothing): every (path, tune set) pair smoothed to a target rms, the weight searched on the device.  NOT EXECUTED in the build container, like the rest of this file.
"pg_tune_set (152 bytes): the smoothing set without a weight (base.lambda must be 0), the dev_rms not to exceed in metres, the first bracket of lambda in m^3, the rounds (1 .. 8), a reserved 0"
struct PgTuneSet
    base::PgSmoothSet
    target::Float64
    lambda_lo::Float64
    lambda_hi::Float64
    rounds::Int32
    reserved::Int32
end
"PgTuneSet() is the library's default; windows, pin_ends and keep_walls as PgSmoothSet takes them"
PgTuneSet(; target=1e-3, lambda_lo=1e-6, lambda_hi=1e3, rounds=3, windows=(), pin_ends=false, keep_walls=false) =
    PgTuneSet(PgSmoothSet(; windows=windows, pin_ends=pin_ends, keep_walls=keep_walls), Float64(target), Float64(lambda_lo), Float64(lambda_hi), Int32(rounds), Int32(0))
"pg_tune_stats (72 bytes), one per (path, set) pair: the chosen weight, the last bracket, dev_rms at its ends, the verdict (0 bracketed, -1 dev_rms(lambda_lo) > target, +1 dev_rms(lambda_hi) <= target), the rounds that evaluated, whether dev_rms was non-decreasing along every ladder"
struct PgTuneStats
    lambda::Float64
    lo::Float64
    hi::Float64
    rms_lo::Float64
    rms_hi::Float64
    verdict::Float64
    rounds_done::Float64
    monotone::Float64
    reserved::Float64
end
"specs and waypoints as smooth_waypoints! takes them -> (waypoints_out [n_wp_total, n_sets], stats [n_sets, n_path], tune [n_sets, n_path]): column k is the whole waypoint array under set k with the weight the search chose"
function tune_smoothing!(mpc::BatchedTrajectoryTrackingMPC, specs::Vector{PgFitSpec}, waypoints::Vector{PgWaypoint}, sets::Vector{PgTuneSet})
    (sizeof(PgTuneSet), sizeof(PgTuneStats), sizeof(PgSmoothStats)) == (152, 72, 72) || error("PigeonMI355X.jl: the pg_tune_smoothing structures differ from include/pigeon_mpc.h")
    n, ns, nw = length(specs), length(sets), length(waypoints)
    out = Matrix{PgWaypoint}(undef, nw, ns); stats = Matrix{PgSmoothStats}(undef, ns, n); tune = Matrix{PgTuneStats}(undef, ns, n)
    check(mpc, ccall(sym(mpc, :pg_tune_smoothing), Cint, (Ptr{Cvoid}, Int32, Ptr{PgFitSpec}, Int32, Ptr{PgWaypoint}, Int32, Ptr{PgTuneSet}, Ptr{PgWaypoint}, Ptr{PgSmoothStats}, Ptr{PgTuneStats}),
                     mpc.handle, Int32(n), specs, Int32(nw), waypoints, Int32(ns), sets, out, stats, tune), "pg_tune_smoothing")
    out, stats, tune
end
"{ default_smooth_set, 1e-3, 1e-6, 1e3, 3, 0 } as the library states them (pg_default_tune_set)"
default_tune_set(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_tune_set), PgTuneSet, ())

# The line inside the tube (pg_optimize_line): every (path, line set) pair moved along its normals to the least bending energy the walls allow.  NOT EXECUTED in the build container, like the rest of this file.
"pg_line_set (176 bytes): mu and rho in 1/m^3 (scale both by 1 / h_mean^3 of the path), the margin to each edge, the largest move, the stopping tolerance, up to four windows in the cumulative chord length with their own margin or a pin, iters (1 .. 4096), the flags, two reserved zeros"
struct PgLineSet
    mu::Float64
    rho::Float64
    margin::Float64
    alpha_max::Float64
    tol::Float64
    u_lo::NTuple{4,Float64}
    u_hi::NTuple{4,Float64}
    win_margin::NTuple{4,Float64}
    win_pin::NTuple{4,Int32}
    iters::Int32
    n_win::Int32
    pin_ends::Int32
    keep_walls::Int32
    reserved::NTuple{2,Int32}
end
"PgLineSet(h_mean=3.74) is mu = 1e-6 / h^3, rho = 0.1 / h^3; windows: (u_lo, u_hi, margin, pin) entries"
function PgLineSet(; h_mean=1.0, mu=1e-6, rho=0.1, margin=0.5, alpha_max=2.0, tol=0.0, iters=1000, windows=(), pin_ends=false, keep_walls=false)
    length(windows) <= 4 || error("PgLineSet: at most 4 windows")
    pad(f, d) = ntuple(j -> j <= length(windows) ? f(windows[j]) : d, 4)
    PgLineSet(mu / h_mean^3, rho / h_mean^3, margin, alpha_max, tol, pad(w -> Float64(w[1]), 0.0), pad(w -> Float64(w[2]), 0.0), pad(w -> Float64(w[3]), 0.0), pad(w -> Int32(w[4] ? 1 : 0), Int32(0)),
              Int32(iters), Int32(length(windows)), Int32(pin_ends), Int32(keep_walls), (Int32(0), Int32(0)))
end
"pg_line_stats (96 bytes), one per (path, set) pair: J(0) and J(alpha), the largest |alpha| and its waypoint, the waypoints at a bound, both residuals of the last iteration, the iterations done, the smallest pivot, the smallest chord and width of the output"
struct PgLineStats
    bend_in::Float64
    bend_out::Float64
    alpha_abs_max::Float64
    i_alpha_max::Float64
    n_active::Float64
    r_prim::Float64
    r_dual::Float64
    iters_done::Float64
    pivot_min::Float64
    chord_min::Float64
    width_min::Float64
    reserved::Float64
end
"specs and waypoints as smooth_waypoints! takes them -> (waypoints_out [n_wp_total, n_sets], stats [n_sets, n_path]): column k is the whole waypoint array under set k"
function optimize_line!(mpc::BatchedTrajectoryTrackingMPC, specs::Vector{PgFitSpec}, waypoints::Vector{PgWaypoint}, sets::Vector{PgLineSet})
    (sizeof(PgLineSet), sizeof(PgLineStats)) == (176, 96) || error("PigeonMI355X.jl: the pg_optimize_line structures differ from include/pigeon_mpc.h")
    n, ns, nw = length(specs), length(sets), length(waypoints)
    out = Matrix{PgWaypoint}(undef, nw, ns); stats = Matrix{PgLineStats}(undef, ns, n)
    check(mpc, ccall(sym(mpc, :pg_optimize_line), Cint, (Ptr{Cvoid}, Int32, Ptr{PgFitSpec}, Int32, Ptr{PgWaypoint}, Int32, Ptr{PgLineSet}, Ptr{PgWaypoint}, Ptr{PgLineStats}),
                     mpc.handle, Int32(n), specs, Int32(nw), waypoints, Int32(ns), sets, out, stats), "pg_optimize_line")
    out, stats
end
"{ 1e-6, 0.1, 0.5, 2, 0, no windows, 1000, 0, 0, 0 } as the library states them (pg_default_line_set)"
default_line_set(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_line_set), PgLineSet, ())

# Making the starts (pg_make_starts): the inputs of a batch placed on the installed trajectory library on the device.  NOT EXECUTED in the build container, like the rest of this file.
"pg_start_set (240 bytes): 13 uniform ranges (lo, hi) in the order of the draws, then the modes and three reserved zeros"
struct PgStartSet
    s_lo::Float64; s_hi::Float64
    e_lo::Float64; e_hi::Float64
    dpsi_lo::Float64; dpsi_hi::Float64
    v_lo::Float64; v_hi::Float64
    uy_lo::Float64; uy_hi::Float64
    dr_lo::Float64; dr_hi::Float64
    delta_lo::Float64; delta_hi::Float64
    fx_lo::Float64; fx_hi::Float64
    dt0_lo::Float64; dt0_hi::Float64
    other_dx_lo::Float64; other_dx_hi::Float64
    other_dy_lo::Float64; other_dy_hi::Float64
    other_dpsi_lo::Float64; other_dpsi_hi::Float64
    other_v_lo::Float64; other_v_hi::Float64
    s_mode::Int32
    e_mode::Int32
    steady::Int32
    time_mode::Int32
    other_mode::Int32
    reserved::NTuple{3,Int32}
end
"every range [0, 0] except v = [1, 1], every mode 0, as the library states them (pg_default_start_set)"
default_start_set(mpc::BatchedTrajectoryTrackingMPC) = ccall(sym(mpc, :pg_default_start_set), PgStartSet, ())
"sets, the set of every instance (0-based, as in C; nothing: set 0), a seed and the stream id of every instance (nothing: its position) -> (state [6, B], control [3, B], t0 [B], other [4, B], time_offset [B], placed [4, B] = s, e, dpsi, V(s)); install = true leaves the handle as pg_set_inputs with these arrays would"
function make_starts!(mpc::BatchedTrajectoryTrackingMPC, B::Integer, sets::Vector{PgStartSet}; index::Union{Nothing,Vector{Int32}}=nothing, seed::Integer=0,
                      streams::Union{Nothing,Vector{UInt64}}=nothing, install::Bool=true)
    (sizeof(PgStartSet), fieldoffset(PgStartSet, 27)) == (240, 208) || error("PigeonMI355X.jl: PgStartSet differs from pg_start_set of include/pigeon_mpc.h")
    (index === nothing || length(index) == B) && (streams === nothing || length(streams) == B) || error("make_starts!: index and streams have B entries")
    state = zeros(Float64, 6, B); control = zeros(Float64, 3, B); t0 = zeros(Float64, B); other = zeros(Float64, 4, B); toff = zeros(Float64, B); placed = zeros(Float64, 4, B)
    check(mpc, ccall(sym(mpc, :pg_make_starts), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{PgStartSet}, Ptr{Int32}, UInt64, Ptr{UInt64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                     mpc.handle, Int32(B), Int32(length(sets)), sets, index === nothing ? Ptr{Int32}(C_NULL) : index, UInt64(seed), streams === nothing ? Ptr{UInt64}(C_NULL) : streams,
                     Int32(install), state, control, t0, other, toff, placed), "pg_make_starts")
    state, control, t0, other, toff, placed
end

"mpc.solved = false (src/ros_integration.jl:34,41,147)"
reset!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_reset), Cint, (Ptr{Cvoid}, Ptr{UInt8}), mpc.handle, C_NULL), "pg_reset")

# ---- the five generic functions of the reference, same names, same order --------------------------------------------------------
function compute_time_steps!(mpc::BatchedTrajectoryTrackingMPC, t0::AbstractVector{Float64})
    mpc.t .= t0
    # Vector{BicycleState{Float64}} is B x 6 doubles, instance-major: exactly the layout the ABI expects
    check(mpc, ccall(sym(mpc, :pg_set_inputs), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                            mpc.handle, mpc.B, mpc.current_state, mpc.current_control, mpc.t, mpc.other_car_state, mpc.time_offset), "pg_set_inputs")
    check(mpc, ccall(sym(mpc, :pg_compute_time_steps), Cint, (Ptr{Cvoid},), mpc.handle), "pg_compute_time_steps")
end
compute_linearization_nodes!(mpc::BatchedTrajectoryTrackingMPC) =
    check(mpc, ccall(sym(mpc, :pg_compute_linearization_nodes), Cint, (Ptr{Cvoid},), mpc.handle), "pg_compute_linearization_nodes")
update_QP!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_update_qp), Cint, (Ptr{Cvoid},), mpc.handle), "pg_update_qp")
solve!(mpc::BatchedTrajectoryTrackingMPC) = check(mpc, ccall(sym(mpc, :pg_solve), Cint, (Ptr{Cvoid},), mpc.handle), "pg_solve")
function get_next_control(mpc::BatchedTrajectoryTrackingMPC)
    u = Vector{BicycleControl{Float64}}(undef, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_next_control), Cint, (Ptr{Cvoid}, Ptr{Float64}), mpc.handle, u), "pg_get_next_control")
    u
end

"The control the ROS loop sends (src/ros_integration.jl:114-124): HJI fallback policy optimal_control(...) when V <= HJI_ϵ in trajectory mode, else the MPC control"
function get_next_control(mpc::BatchedTrajectoryTrackingMPC, use_HJI_policy::Bool)
    u = Vector{BicycleControl{Float64}}(undef, mpc.B); source = Vector{Int32}(undef, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_next_control_hji), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
                            mpc.handle, use_HJI_policy, u, source, C_NULL), "pg_get_next_control_hji")
    u, source            # source: 0 MPC, 1 HJI policy ("with a hammer"), 2 unsafe but policy off ("with a feather")
end

"simulate(mpc, q0, u0, N) (src/model_predictive_control.jl:80-100) for the whole batch, closed loop resident on the GPU"
function simulate!(mpc::BatchedTrajectoryTrackingMPC, steps::Integer; dt=0.01)
    check(mpc, ccall(sym(mpc, :pg_simulate_dev), Cint, (Ptr{Cvoid}, Int32, Float64, Ptr{Cvoid}, Ptr{Cvoid}), mpc.handle, steps, dt, C_NULL, C_NULL), "pg_simulate_dev")
    check(mpc, ccall(sym(mpc, :pg_get_state), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), mpc.handle, mpc.current_state, mpc.current_control, mpc.t), "pg_get_state")
    mpc.current_state, mpc.current_control
end

const HUMAN_MODES = Dict(:hold => Int32(0), :worst => Int32(1), :script => Int32(2))

"""simulate! with the control the ROS loop sends fed back (src/ros_integration.jl:114-124) against an other car that moves (pg_simulate_safety_dev): human = :hold
((ω, a) = (0, 0)), :worst (optimal_disturbance, src/HJI_computation.jl:90-131) or :script (human_u_dev: a device array [steps][B][2] of the library's element type).
Not executed here (no Julia toolchain); the Python mirror simulate_safety_ and tests/test_gpu_safety_rollout.py exercise the same ABI."""
function simulate_safety!(mpc::BatchedTrajectoryTrackingMPC, steps::Integer; dt=0.01, use_HJI_policy::Bool=true, human::Symbol=:hold, human_u_dev::Ptr{Cvoid}=C_NULL)
    check(mpc, ccall(sym(mpc, :pg_simulate_safety_dev), Cint, (Ptr{Cvoid}, Int32, Float64, Int32, Int32, Ptr{Cvoid}, ntuple(_ -> Ptr{Cvoid}, 6)...),
                     mpc.handle, steps, dt, use_HJI_policy, HUMAN_MODES[human], human_u_dev, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL), "pg_simulate_safety_dev")
    check(mpc, ccall(sym(mpc, :pg_get_state), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), mpc.handle, mpc.current_state, mpc.current_control, mpc.t), "pg_get_state")
    check(mpc, ccall(sym(mpc, :pg_get_safety_state), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                     mpc.handle, mpc.other_car_state, C_NULL, C_NULL, C_NULL), "pg_get_safety_state")
    mpc.current_state, mpc.current_control, mpc.other_car_state
end

"Per controller since the rollout's clock last restarted: (V_min, first step index with V <= 0 or -1, steps on the HJI policy)"
function safety_summary(mpc::BatchedTrajectoryTrackingMPC)
    V_min = Vector{Float64}(undef, mpc.B); first_breach = Vector{Int32}(undef, mpc.B); policy_steps = Vector{Int32}(undef, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_safety_state), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                     mpc.handle, C_NULL, V_min, first_breach, policy_steps), "pg_get_safety_state")
    V_min, first_breach, policy_steps
end

"""from_autobox_callback (src/ros_integration.jl:48-151) for every controller on the installed inputs (pg_node_step_dev): the gates (pre_flag, the trajectory-time window,
Ux < 1), the compute calls, the selection and the NaN fallback.  current_control plays the to_autobox message and holds the message after the callback on return.
pre_flag_dev, cmd_out_dev, se_out_dev, event_dev: device arrays or C_NULL (pre_flag [B] UInt8; cmd [B][3], se [B][2] of the library's element type; event [B] Int32).
Not executed here (no Julia toolchain); the Python mirror node_step_ and tests/test_gpu_node.py exercise the same ABI."""
function from_autobox_step!(mpc::BatchedTrajectoryTrackingMPC; use_HJI_policy::Bool=false, pre_flag_dev::Ptr{Cvoid}=C_NULL, cmd_out_dev::Ptr{Cvoid}=C_NULL,
                            se_out_dev::Ptr{Cvoid}=C_NULL, event_dev::Ptr{Cvoid}=C_NULL)
    check(mpc, ccall(sym(mpc, :pg_node_step_dev), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                     mpc.handle, use_HJI_policy, pre_flag_dev, cmd_out_dev, se_out_dev, event_dev), "pg_node_step_dev")
    check(mpc, ccall(sym(mpc, :pg_get_state), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), mpc.handle, mpc.current_state, mpc.current_control, mpc.t), "pg_get_state")
    mpc.current_control
end

"""The node's closed loop (pg_simulate_node_dev): simulate_safety! with the node's gates and NaN fallback, the plant driven by the command last published (the applied
command).  pre_flag_dev: a device array [steps][B] UInt8 or C_NULL (engaged).  Returns (state, message, other car, applied command); node_state gives heartbeat and counts.
Not executed here (no Julia toolchain); the Python mirror simulate_node_ and tests/test_gpu_node.py exercise the same ABI."""
function simulate_node!(mpc::BatchedTrajectoryTrackingMPC, steps::Integer; dt=0.01, use_HJI_policy::Bool=false, human::Symbol=:hold, human_u_dev::Ptr{Cvoid}=C_NULL,
                        pre_flag_dev::Ptr{Cvoid}=C_NULL)
    check(mpc, ccall(sym(mpc, :pg_simulate_node_dev), Cint, (Ptr{Cvoid}, Int32, Float64, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, ntuple(_ -> Ptr{Cvoid}, 4)...),
                     mpc.handle, steps, dt, use_HJI_policy, HUMAN_MODES[human], human_u_dev, pre_flag_dev, C_NULL, C_NULL, C_NULL, C_NULL), "pg_simulate_node_dev")
    check(mpc, ccall(sym(mpc, :pg_get_state), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), mpc.handle, mpc.current_state, mpc.current_control, mpc.t), "pg_get_state")
    check(mpc, ccall(sym(mpc, :pg_get_safety_state), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                     mpc.handle, mpc.other_car_state, C_NULL, C_NULL, C_NULL), "pg_get_safety_state")
    applied, _, _ = node_state(mpc)
    mpc.current_state, mpc.current_control, mpc.other_car_state, applied
end

"Per controller: applied command [3, B], heartbeat (callbacks that computed), counts [4, B] (pre_flag off, outside the window, low speed, NaN fallback since the clock restarted)"
function node_state(mpc::BatchedTrajectoryTrackingMPC)
    applied = Matrix{Float64}(undef, 3, mpc.B); heartbeat = Vector{Int32}(undef, mpc.B); counts = Matrix{Int32}(undef, 4, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_node_state), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}), mpc.handle, applied, heartbeat, counts), "pg_get_node_state")
    applied, heartbeat, counts
end

"Outcome of the active-set polish per instance: k >= 1 verified in round k (exact optimum on its active set), 0 not run, -1 not verified"
function polish_info(mpc::BatchedTrajectoryTrackingMPC)
    p = Vector{Int32}(undef, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_polish_info), Cint, (Ptr{Cvoid}, Ptr{Int32}), mpc.handle, p), "pg_get_polish_info")
    p
end

"Multipliers of the inequality rows of the last solve, [16, N, B] (column-major view of the ABI's [B][N][16]), indexed like the bits of the active masks"
function multipliers(mpc::BatchedTrajectoryTrackingMPC)
    N = (Int(ccall(sym(mpc, :pg_qp_len), Cint, (Ptr{Cvoid},), mpc.handle)) - 11) ÷ 84          # pg_qp_len = 84 N + 11
    lam = Array{Float64}(undef, 16, N, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_get_multipliers), Cint, (Ptr{Cvoid}, Ptr{Float64}), mpc.handle, lam), "pg_get_multipliers")
    lam
end

"update_QP! inside the solve kernel for step! / simulate! (pg_set_fusion; bit-identical results): mode 0 never (default), 1 always, 2 for all-warm batches"
function set_fusion!(mpc::BatchedTrajectoryTrackingMPC, mode::Integer)
    check(mpc, ccall(sym(mpc, :pg_set_fusion), Cint, (Ptr{Cvoid}, Int32), mpc.handle, Int32(mode)), "pg_set_fusion")
end

"nodes + update_QP! of a large batch with cold instances as one pipelined launch (pg_set_pipeline; bit-identical results): mode 1 where it applies (default), 0 never"
function set_pipeline!(mpc::BatchedTrajectoryTrackingMPC, mode::Integer)
    check(mpc, ccall(sym(mpc, :pg_set_pipeline), Cint, (Ptr{Cvoid}, Int32), mpc.handle, Int32(mode)), "pg_set_pipeline")
end

"build-defined option of the handle by name (pg_set_option: solver rules, launch shape, lateral-solver tuning; the library reads nothing from ENV), e.g. set_option!(mpc, \"graph\", 1)"
function set_option!(mpc::BatchedTrajectoryTrackingMPC, name::AbstractString, value::Real)
    check(mpc, ccall(sym(mpc, :pg_set_option), Cint, (Ptr{Cvoid}, Cstring, Cdouble), mpc.handle, name, Float64(value)), "pg_set_option($name)")
end

"current value of an option, or a read-only launch statistic such as \"stat_pipelined_launches\" (pg_get_option)"
function get_option(mpc::BatchedTrajectoryTrackingMPC, name::AbstractString)
    v = Ref{Cdouble}(0.0)
    check(mpc, ccall(sym(mpc, :pg_get_option), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cdouble}), mpc.handle, name, v), "pg_get_option($name)")
    v[]
end

"number of waiting wavefronts of the pipelined launch that gave up so far (each such step was redone launch per phase: late, not wrong; pg_get_pipeline_fallbacks)"
function pipeline_fallbacks(mpc::BatchedTrajectoryTrackingMPC)
    n = Ref{Int64}(0)
    check(mpc, ccall(sym(mpc, :pg_get_pipeline_fallbacks), Cint, (Ptr{Cvoid}, Ptr{Int64}), mpc.handle, n), "pg_get_pipeline_fallbacks")
    n[]
end

"milliseconds of the last `pg_step_dev` per phase -- (time grid + nodes, update_QP!, solve! + get_next_control) -- the figure `ros_integration.jl:94-109` logs as one number.
The HIP events behind it are OFF by default (four event records cost 13-25 us of stream time per step): call `set_option!(mpc, \"phase_timing\", 1)` first, otherwise
pg_get_phase_ms returns PG_ERR_STATE and its message says that the option is off (pg_get_phase_ms)"
function phase_ms(mpc::BatchedTrajectoryTrackingMPC)
    out = Vector{Float32}(undef, 3)
    check(mpc, ccall(sym(mpc, :pg_get_phase_ms), Cint, (Ptr{Cvoid}, Ptr{Float32}), mpc.handle, out), "pg_get_phase_ms")
    out
end

# per-instance solver status words (include/pigeon_mpc.h: pg_solve_status).  With the polish on, PG_SOLVED is a VERIFIED KKT point of the QP; PG_SOLVED_UNVERIFIED is the
# interior-point iterate no active-set round could verify (a caller that treats it like PG_SOLVED gets the behaviour of earlier versions)
const PG_SOLVED = Int32(1); const PG_MAX_ITER = Int32(2); const PG_NUMERICAL = Int32(3); const PG_INFEASIBLE_X0 = Int32(4); const PG_SOLVED_UNVERIFIED = Int32(5)
is_solved(status::Integer) = status == PG_SOLVED || status == PG_SOLVED_UNVERIFIED

"update_HJI_values_marker! / update_HJI_contour_marker! (src/rviz.jl:23-40,60-69) for a batch of relative states q (7 x B): V at every (x, y) knot pair of grid
dimensions 1, 2 and the zero-level crossings on the grid edges (NaN = none)"
function hji_value_slice(mpc::BatchedTrajectoryTrackingMPC, q::Matrix{Float64})
    dims = Vector{Int32}(undef, 7)
    check(mpc, ccall(sym(mpc, :pg_hji_grid_dims), Cint, (Ptr{Cvoid}, Ptr{Int32}), mpc.handle, dims), "pg_hji_grid_dims")
    n1, n2, B = dims[1], dims[2], size(q, 2)
    V = Array{Float64}(undef, n2, n1, B); cx = Array{Float64}(undef, n2, n1 - 1, B); cy = Array{Float64}(undef, n2 - 1, n1, B)     # column-major views of [B][n1][n2] etc.
    check(mpc, ccall(sym(mpc, :pg_hji_slice), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), mpc.handle, B, q, V, C_NULL, cx, cy),
          "pg_hji_slice")
    V, cx, cy
end

"The convenience entry points named in the project brief: all five calls for every instance."
function step!(mpc::BatchedTrajectoryTrackingMPC, t0::AbstractVector{Float64})
    u = Vector{BicycleControl{Float64}}(undef, mpc.B); status = Vector{Int32}(undef, mpc.B); iters = Vector{Int32}(undef, mpc.B)
    check(mpc, ccall(sym(mpc, :pg_step), Cint,
                            (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                            mpc.handle, mpc.B, mpc.current_state, mpc.current_control, t0, mpc.other_car_state, mpc.time_offset, u, status, iters), "pg_step")
    u, status, iters
end
const MPC! = step!

# ---- multi-GPU (SURVEY 8e): the batch shards by instance, one handle per device, no data-path collective --------------------------------------------------------
# One Julia process drives every GPU of the node through its own handle (pg_config.device); the step of every shard is queued asynchronously (pg_set_inputs +
# pg_step_dev return once the work is on the device's stream) before any result is waited for, and the gather of the B x 3 controls is the concatenation of the shards'
# host read-backs -- the ROS publishers want them in host memory anyway.  (bench.py's one-process-per-GPU harness gathers on the devices with RCCL instead.)
"Instances [lo, hi] (1-based, inclusive) of shard `g` of `G`: contiguous blocks, the remainder spread over the first shards (pigeon.jl_amd/sharding.py: shard_range)"
function shard_range(B::Integer, G::Integer, g::Integer)
    base, rem = divrem(B, G)
    lo = (g - 1) * base + min(g - 1, rem)
    lo + 1, lo + base + (g <= rem ? 1 : 0)
end

struct ShardedTrajectoryTrackingMPC
    shards::Vector{BatchedTrajectoryTrackingMPC}
    ranges::Vector{UnitRange{Int}}
    B::Int
end

"B controllers spread over `devices` (device ordinals); `make(B_g, device)` builds one shard, e.g. (b, d) -> BatchedTrajectoryTrackingMPC(X1(), traj, b; device = d)"
function ShardedTrajectoryTrackingMPC(make::Function, B::Integer, devices::AbstractVector{<:Integer})
    G = length(devices)
    ranges = [UnitRange(shard_range(B, G, g)...) for g in 1:G]
    ShardedTrajectoryTrackingMPC([make(length(ranges[g]), devices[g]) for g in 1:G], ranges, B)
end

"All five calls for every instance on every GPU: states / controls / t0 are the full-batch vectors; returns (u, status, iters) of the full batch"
function step!(s::ShardedTrajectoryTrackingMPC, current_state::Vector{BicycleState{Float64}}, current_control::Vector{BicycleControl{Float64}}, t0::Vector{Float64})
    for (mpc, r) in zip(s.shards, s.ranges)          # queue every shard's step first ...
        mpc.current_state .= view(current_state, r); mpc.current_control .= view(current_control, r); mpc.t .= view(t0, r)
        check(mpc, ccall(sym(mpc, :pg_set_inputs), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                mpc.handle, mpc.B, mpc.current_state, mpc.current_control, mpc.t, mpc.other_car_state, mpc.time_offset), "pg_set_inputs")
        check(mpc, ccall(sym(mpc, :pg_step_dev), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), mpc.handle, C_NULL), "pg_step_dev")
    end
    u = Vector{BicycleControl{Float64}}(undef, s.B); status = Vector{Int32}(undef, s.B); iters = Vector{Int32}(undef, s.B)
    for (mpc, r) in zip(s.shards, s.ranges)          # ... then gather: each read-back waits for its own device only
        ug = get_next_control(mpc); st = Vector{Int32}(undef, mpc.B); it = Vector{Int32}(undef, mpc.B)
        check(mpc, ccall(sym(mpc, :pg_get_solve_info), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt16}, Ptr{Float64}), mpc.handle, st, it, C_NULL, C_NULL), "pg_get_solve_info")
        u[r] .= ug; status[r] .= st; iters[r] .= it
    end
    u, status, iters
end

end # module
