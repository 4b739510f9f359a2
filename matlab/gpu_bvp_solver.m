% gpu_bvp_solver.m
% Shim for libocs.so (include/ocs.h); replaces the reference's functions/bvp_solver.m.
% NOT VERIFIED: no MATLAB or Octave exists in the build pipeline; the same call sequence is tested through
% Python ctypes (tests/test_gpu_bvp_solver.py).  See INTEGRATION.md.
% The boundary-value problem is collocated on the nodes of tspan (a fixed mesh: bvp5c's mesh adaptation is a toolbox; refine
% tspan for accuracy) and solved by a damped Newton iteration on the device.  prob.bcFunc / yLJac / yRJac / optJac are not
% supported.  options.y0 here: 2 nS x numel(tspan) samples or a function handle t -> 2 nS x k; options.u0: nC x (2N+1) samples
% on the integrator grid or a function handle.
function soln = gpu_bvp_solver(prob, x0, tspan, options)                       % bvp_solver.m:1
   integ = GpuRK4Integrator(tspan);  o = libstruct('ocs_bvp_options');
   calllib('libocs', 'ocs_bvp_default_options', o);                           % :20 nINTERP_PTS; NewtonTol, MaxIter, maxBacktracks
   names = {'nINTERP_PTS', 'NewtonTol', 'MaxIter', 'maxBacktracks'};
   if nargin < 4, options = struct(); end
   for k = 1:numel(names)
      if isfield(options, names{k}), o.(names{k}) = options.(names{k}); end
   end
   ignored = intersect(fieldnames(options), {'bvpRelTol', 'bvpAbsTol', 'MAX_MESH_SIZE', 'RelTol', 'AbsTol'});
   if ~isempty(ignored)                                                       % :15-19: they steer bvp5c / odevr7
      warning('gpu_bvp_solver:ignored', '%s have no effect: the mesh is tspan, Newton stops at NewtonTol', strjoin(ignored', ', '));
   end
   N = numel(tspan) - 1;  nS = numel(x0);  nC = size(prob.ControlBounds, 1);
   y0 = [];  u0 = [];
   if isfield(options, 'y0')                                                  % :91-93
      y0 = options.y0;  if isa(y0, 'function_handle'), y0 = y0(tspan(:)'); end
   elseif isfield(options, 'u0')                                              % :94-97
      u0 = options.u0;  if isa(u0, 'function_handle'), u0 = u0(integ.t(:)'); end
   end
   y = zeros(2*nS, N+1);  x = zeros(nS, N+1);  lam = x;  uI = zeros(nC, o.nINTERP_PTS);  J = 0;
   iters = int32(0);  conv = int32(0);  res = 0;
   [rc, ~, ~, ~, ~, ~, ~, y, x, lam, uI, J, iters, conv, res] = calllib('libocs', 'ocs_bvp_solver', integ.hnd.Value, ...
         prob.h.Value, 1, x0, o, y0, u0, y, x, lam, uI, J, iters, conv, res);
   if rc < 0, ocs_check(rc); end   % bad options, unsupported problem, HIP error; rc > 0 = OCS_NUM_NOT_CONVERGED
   soln = struct();
   if conv > 0
      interpPts = linspace(tspan(1), tspan(end), o.nINTERP_PTS);               % :99
      soln.u = vectorInterpolant(interpPts, uI, 'pchip');                      % :126
      soln.x = vectorInterpolant(tspan, x, 'pchip');  soln.lam = vectorInterpolant(tspan, lam, 'pchip');  soln.J = J;   % :132
      soln.y = y;  soln.iterations = iters;  soln.resnorm = res;
   end
end
